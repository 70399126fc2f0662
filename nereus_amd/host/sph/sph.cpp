// sph.cpp — Nereus::SPH over the nrs_* C ABI (libnereus_hip.so).
//
// What each method has to do is defined by the reference's sph/sph.cpp (constructor defaults :29-93,
// _initialize :132-188, update :215-285, updateGrid :313-337, addNewParticle :341-368,
// generateParticleCube :373-386, updateGpuBoundaries :391-432).  How it is done here differs: no per-step
// PCIe copies (state stays on the GPU, host arrays are refreshed when somebody asks for them), run-time
// capacity instead of MAX_PARTICLE_NUMBER, idempotent _initialize().
#include "sph.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "nereus_hip.h"

NEREUS_NAMESPACE_BEGIN

namespace {

// Smoothing-kernel factors.  The three flavours differ only in where M_PI is narrowed to SReal:
// 0 = SPH::SPH() (sph.cpp:76-90), 1 = IISPH::IISPH() (iisph.cpp:70-80), 2 = the SphSimParams constructors.
void kernelFactors(SphSimParams &p, int flavour)
{
    const SReal h = p.interactionRadius;
    const float h3 = powf(h, 3.0), h6 = powf(h, 6.0), h9 = powf(h, 9.0);
    if (flavour == 1) {
        p.kpoly = 315.0 / (64.0 * M_PI * h9);
        p.kpoly_grad = -945.0 / (32.0 * M_PI * h9);
        p.kpress_grad = -45.0 / (M_PI * h6);
        p.kvisc_grad = 15.0 / (2 * M_PI * h3);
        p.ksurf1 = 32.0 / (M_PI * h9);
    } else {
        const SReal pi = (SReal)M_PI;
        p.kpoly = 315.0 / (64.0 * pi * h9);
        p.kpoly_grad = -945.0 / (32.0 * pi * h9);
        p.kpress_grad = -45.0 / (pi * h6);
        p.kvisc_grad = (flavour == 0) ? 15.0 / (2.0 * pi * h3) : 15.0 / (2 * pi * h3);
        p.ksurf1 = 32.0 / (pi * h9);
    }
    p.kvisc_denum = 2.0 * h3;
    p.ksurf2 = h6 / 64.0;
    p.bpol = 0.007f / (powf(h, 3.25));
}

SReal defaultSoundSpeed()
{
    const SReal eta = 0.01, H = 0.1;
    const SReal vf = std::sqrt(2.0 * 9.81 * H);
    return vf / (std::sqrt(eta));
}

SUint nextPow2(SUint v)
{
    v--;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return v + 1;
}

SUint envCapacity()
{
    const char *e = std::getenv("NEREUS_CAPACITY");
    if (e && *e) {
        const long long v = std::atoll(e);
        if (v > 0) return (SUint)std::min<long long>(v, (1ll << 30) - 1);
    }
    return MAX_PARTICLE_NUMBER;
}

} // namespace

void nereusKernelFactors(SphSimParams &p, int flavour) { kernelFactors(p, flavour); }
SReal nereusDefaultSoundSpeed() { return defaultSoundSpeed(); }

SPH::SPH()
    : m_gridSortBits(32), m_pos(nullptr), m_vel(nullptr), m_density(nullptr), m_pressure(nullptr), m_forces(nullptr),
      m_colors(nullptr), m_numParticles(0), m_hostCapacity(0), m_bi(nullptr), m_vbi(nullptr), m_num_boundaries(0),
      m_ctx(nullptr), m_ctxCapacity(0), m_hostDirty(true), m_deviceNewer(false), m_boundariesPending(false), m_numBodies(0),
      m_eagerSync(false), m_initialized(false), m_cfl(false), m_cflLambda(0.4f), m_asyncReadback(false),
      m_framesInFlight(0), m_frame(nullptr), m_frameCount(0), m_frameStep(0), m_frameIsCurrent(false)
{
    std::cout << GREEN << "construction of sph based system" << RESET << std::endl;
    std::memset(&m_params, 0, sizeof(m_params));
    m_params.gasStiffness = 800;
    m_params.restDensity = 1000;
    m_params.particleRadius = 0.02;
    m_params.timestep = 1E-3;
    m_params.viscosity = 0.005;
    m_params.surfaceTension = 0.01;
    m_params.gravity = make_SVec3(0., -9.81, 0.);
    m_params.interactionRadius = 0.0457;
    m_params.particleMass = 0.5 * powf(m_params.interactionRadius, 3) * m_params.restDensity;
    m_params.beta = 450.0;
    m_params.soundSpeed = defaultSoundSpeed();
    m_params.worldOrigin = make_SVec3(-1.1, -1.1, -1.1);
    m_params.gridSize = make_uint3(64, 64, 64);
    const SReal h = m_params.interactionRadius;
    m_params.cellSize = make_SVec3(h, h, h);
    m_params.numCells = m_params.gridSize.x * m_params.gridSize.y * m_params.gridSize.z;
    kernelFactors(m_params, 0);
    _initialize();
    m_numParticles = 0;
}

SPH::SPH(SphSimParams params)
    : m_params(params), m_gridSortBits(32), m_pos(nullptr), m_vel(nullptr), m_density(nullptr), m_pressure(nullptr),
      m_forces(nullptr), m_colors(nullptr), m_numParticles(0), m_hostCapacity(0), m_bi(nullptr), m_vbi(nullptr),
      m_num_boundaries(0), m_ctx(nullptr), m_ctxCapacity(0), m_hostDirty(true), m_deviceNewer(false),
      m_boundariesPending(false), m_numBodies(0), m_eagerSync(false), m_initialized(false), m_cfl(false), m_cflLambda(0.4f), m_asyncReadback(false),
      m_framesInFlight(0), m_frame(nullptr), m_frameCount(0), m_frameStep(0), m_frameIsCurrent(false)
{
    kernelFactors(m_params, 2);
    _initialize();
    m_numParticles = 0;
}

SPH::~SPH()
{
    releaseContext();
    std::free(m_pos); std::free(m_vel); std::free(m_density); std::free(m_pressure); std::free(m_forces);
    std::free(m_colors);
}

void SPH::fatal(const char *what) const
{
    std::fprintf(stderr, "Nereus: %s: %s\n", what, nrs_last_error());
    std::exit(EXIT_FAILURE); // same policy as the reference's checkCudaErrors
}

int SPH::solverKind() const { return NRS_SOLVER_SESPH; }

void SPH::growHost(SUint capacity)
{
    if (capacity <= m_hostCapacity) return;
    auto grow = [&](SReal *&a, size_t per) {
        SReal *n = (SReal *)std::realloc(a, sizeof(SReal) * per * capacity);
        if (!n) { std::fprintf(stderr, "Nereus: out of host memory\n"); std::exit(EXIT_FAILURE); }
        std::memset(n + per * m_hostCapacity, 0, sizeof(SReal) * per * (capacity - m_hostCapacity));
        a = n;
    };
    grow(m_pos, 4); grow(m_vel, 4); grow(m_forces, 4); grow(m_colors, 4);
    grow(m_density, 1); grow(m_pressure, 1);
    m_hostCapacity = capacity;
}

void SPH::_initialize()
{
    // The reference allocates here every time it is called (constructor, derived constructor, main.cpp:534)
    // and leaks the earlier allocations; this one only makes sure storage exists.  The device context is
    // created lazily so that it sees the final parameters and solver kind.
    if (!m_initialized) {
        growHost(envCapacity());
        m_initialized = true;
    }
}

void SPH::_finalize() { synchronize(); }

void SPH::_initializeGrid()
{
    // cell tables are (re)allocated by the device library when it sees a new numCells (nrs_set_params)
}

void SPH::reserveParticles(SUint capacity)
{
    growHost(capacity);
    if (m_ctx && capacity > m_ctxCapacity) {
        pullDeviceToHost();
        trackSave();
        releaseContext();
        m_hostDirty = true;
    }
}

void SPH::releaseContext()
{
    if (m_ctx) {
        nrs_destroy(m_ctx); // also frees the pinned frames
        m_ctx = nullptr;
        m_ctxCapacity = 0;
        m_framesInFlight = 0;
        m_frame = nullptr;
        m_frameIsCurrent = false;
        if (m_num_boundaries) m_boundariesPending = true;
    }
}

void SPH::ensureContext()
{
    if (m_ctx && m_ctxCapacity >= m_numParticles) return;
    if (m_ctx) { // capacity exceeded: save the state and rebuild a larger context
        pullDeviceToHost();
        trackSave();
        releaseContext();
        m_hostDirty = true;
    }
    nrs_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    cfg.device = -1;
    cfg.solver = solverKind();
    cfg.precision = (int)sizeof(SReal) * 8;
    cfg.kernel_set = KERNEL_SET;
    cfg.surface_tension = USE_SURFACE_TENSION;
    cfg.flags = std::getenv("NEREUS_REFERENCE_ORDER") ? NRS_FLAG_REFERENCE_ORDER : 0;
    cfg.capacity = std::max<SUint>(m_hostCapacity, m_numParticles);
    if (nrs_create(&cfg, &m_params, &m_ctx) != NRS_OK) fatal("nrs_create");
    m_ctxCapacity = (SUint)cfg.capacity;
    m_trackPending = m_tracking; // enabled behind the first upload (trackStart)
    configureContext();
    if (m_boundariesPending && m_bi && m_vbi && m_num_boundaries) {
        if (nrs_set_boundaries(m_ctx, m_bi, m_vbi, m_num_boundaries, 0) != NRS_OK) fatal("nrs_set_boundaries");
        m_boundariesPending = false;
        if (!m_bodyOf.empty() && nrs_set_boundary_bodies(m_ctx, m_bodyOf.data(), m_bodyOf.size(), m_numBodies) != NRS_OK)
            fatal("nrs_set_boundary_bodies");
    }
}

void SPH::setBoundaryBodies(const SUint *bodyOf, SUint nbodies)
{
    ensureContext();
    if (nrs_set_boundary_bodies(m_ctx, bodyOf, bodyOf ? m_num_boundaries : 0, nbodies) != NRS_OK) fatal("nrs_set_boundary_bodies");
    if (bodyOf && nbodies > 1) m_bodyOf.assign(bodyOf, bodyOf + m_num_boundaries);
    else m_bodyOf.clear();
    m_numBodies = m_bodyOf.empty() ? 0 : nbodies;
}
void SPH::setBodyVelocity(SUint body, const double v[3], const double omega[3])
{
    ensureContext();
    if (nrs_set_body_velocity(m_ctx, body, v, omega) != NRS_OK) fatal("nrs_set_body_velocity");
}
void SPH::setBodyPose(SUint body, const double x[3], const double q[4])
{
    ensureContext();
    if (nrs_set_body_pose(m_ctx, body, x, q) != NRS_OK) fatal("nrs_set_body_pose");
}
void SPH::getBodyPose(SUint body, double x[3], double q[4])
{
    ensureContext();
    if (nrs_get_body_pose(m_ctx, body, x, q) != NRS_OK) fatal("nrs_get_body_pose");
}

// ---- field sampling --------------------------------------------------------------------------------------------------------------
void SPH::sampleLattice(const double origin[3], const double spacing[3], const SUint dims[3], SUint fields)
{
    ensureContext();
    pushHostToDevice();
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.spacing[a] = spacing[a]; L.dims[a] = dims[a]; }
    if (nrs_sample_lattice(m_ctx, &L, fields) != NRS_OK) fatal("nrs_sample_lattice");
}
void SPH::samplePoints(const SVec4 *points, SUint n, SUint fields)
{
    ensureContext();
    pushHostToDevice();
    if (nrs_sample_points(m_ctx, points, n, fields) != NRS_OK) fatal("nrs_sample_points");
}
template <typename T> static void fetchInto(nrs_ctx *ctx, SUint field, std::vector<T> &v, bool &ok)
{
    uint64_t bytes = 0;
    ok = nrs_sample_result(ctx, field, nullptr, 0, &bytes) == NRS_OK;
    if (!ok) return;
    v.resize((size_t)(bytes / sizeof(T)));
    if (bytes) ok = nrs_sample_result(ctx, field, v.data(), bytes, nullptr) == NRS_OK;
}
const std::vector<SReal> &SPH::getSampledDensity()
{
    bool ok = false;
    ensureContext();
    fetchInto(m_ctx, NRS_FIELD_DENSITY, m_sampledDensity, ok);
    if (!ok) fatal("nrs_sample_result");
    return m_sampledDensity;
}
const std::vector<SVec4> &SPH::getSampledGradient()
{
    bool ok = false;
    ensureContext();
    fetchInto(m_ctx, NRS_FIELD_GRADIENT, m_sampledGradient, ok);
    if (!ok) fatal("nrs_sample_result");
    return m_sampledGradient;
}
const std::vector<SVec4> &SPH::getSampledVelocity()
{
    bool ok = false;
    ensureContext();
    fetchInto(m_ctx, NRS_FIELD_VELOCITY, m_sampledVelocity, ok);
    if (!ok) fatal("nrs_sample_result");
    return m_sampledVelocity;
}
const std::vector<SUint> &SPH::getSampledCount()
{
    bool ok = false;
    ensureContext();
    fetchInto(m_ctx, NRS_FIELD_COUNT, m_sampledCount, ok);
    if (!ok) fatal("nrs_sample_result");
    return m_sampledCount;
}

// ---- surface extraction -----------------------------------------------------------------------------------------------------------
void SPH::extractSurface(const double origin[3], const double spacing[3], const SUint dims[3], double iso, SUint flags)
{
    ensureContext();
    pushHostToDevice();
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.spacing[a] = spacing[a]; L.dims[a] = dims[a]; }
    uint64_t V = 0, T = 0;
    if (nrs_surface_extract(m_ctx, &L, iso, flags, &V, &T) != NRS_OK) fatal("nrs_surface_extract");
    m_surfaceV = (SUint)V;
    m_surfaceT = (SUint)T;
}
template <typename T> static void fetchMesh(nrs_ctx *ctx, SUint which, std::vector<T> &v, bool &ok)
{
    uint64_t bytes = 0;
    ok = nrs_surface_result(ctx, which, nullptr, 0, &bytes) == NRS_OK;
    if (!ok) return;
    v.resize((size_t)(bytes / sizeof(T)));
    if (bytes) ok = nrs_surface_result(ctx, which, v.data(), bytes, nullptr) == NRS_OK;
}
const std::vector<SVec4> &SPH::getSurfaceVertices()
{
    bool ok = false;
    ensureContext();
    fetchMesh(m_ctx, NRS_MESH_VERTICES, m_surfaceVertices, ok);
    if (!ok) fatal("nrs_surface_result");
    return m_surfaceVertices;
}
const std::vector<SUint> &SPH::getSurfaceTriangles()
{
    bool ok = false;
    ensureContext();
    fetchMesh(m_ctx, NRS_MESH_TRIANGLES, m_surfaceTriangles, ok);
    if (!ok) fatal("nrs_surface_result");
    return m_surfaceTriangles;
}
const std::vector<SVec4> &SPH::getSurfaceGradient()
{
    bool ok = false;
    ensureContext();
    fetchMesh(m_ctx, NRS_MESH_GRADIENT, m_surfaceGradient, ok);
    if (!ok) fatal("nrs_surface_result");
    return m_surfaceGradient;
}
const std::vector<SVec4> &SPH::getSurfaceVelocity()
{
    bool ok = false;
    ensureContext();
    fetchMesh(m_ctx, NRS_MESH_VELOCITY, m_surfaceVelocity, ok);
    if (!ok) fatal("nrs_surface_result");
    return m_surfaceVelocity;
}

// ---- anisotropic surface reconstruction ---------------------------------------------------------------------------------------------
void SPH::anisoKernels(const nrs_aniso_config *cfg)
{
    ensureContext();
    pushHostToDevice();
    if (nrs_aniso_build(m_ctx, cfg) != NRS_OK) fatal("nrs_aniso_build");
}
template <typename T> static const std::vector<T> &fetchAniso(nrs_ctx *ctx, SUint which, std::vector<T> &v, bool &ok)
{
    uint64_t bytes = 0;
    ok = nrs_aniso_result(ctx, which, nullptr, 0, &bytes) == NRS_OK;
    if (!ok) return v;
    v.resize((size_t)(bytes / sizeof(T)));
    if (bytes) ok = nrs_aniso_result(ctx, which, v.data(), bytes, nullptr) == NRS_OK;
    return v;
}
const std::vector<SVec4> &SPH::getAnisoCenters()
{
    bool ok = false;
    ensureContext();
    fetchAniso(m_ctx, NRS_ANISO_CENTER, m_anisoCenters, ok);
    if (!ok) fatal("nrs_aniso_result");
    return m_anisoCenters;
}
const std::vector<SVec4> &SPH::getAnisoG()
{
    bool ok = false;
    ensureContext();
    fetchAniso(m_ctx, NRS_ANISO_G, m_anisoG, ok);
    if (!ok) fatal("nrs_aniso_result");
    return m_anisoG;
}
const std::vector<SUint> &SPH::getAnisoCount()
{
    bool ok = false;
    ensureContext();
    fetchAniso(m_ctx, NRS_ANISO_COUNT, m_anisoCount, ok);
    if (!ok) fatal("nrs_aniso_result");
    return m_anisoCount;
}
const std::vector<SUint> &SPH::getAnisoIndex()
{
    bool ok = false;
    ensureContext();
    fetchAniso(m_ctx, NRS_ANISO_INDEX, m_anisoIndex, ok);
    if (!ok) fatal("nrs_aniso_result");
    return m_anisoIndex;
}
void SPH::extractSurfaceAniso(const double origin[3], const double spacing[3], const SUint dims[3], double iso, SUint flags, const nrs_aniso_config *cfg)
{
    ensureContext();
    pushHostToDevice();
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.spacing[a] = spacing[a]; L.dims[a] = dims[a]; }
    uint64_t V = 0, T = 0;
    if (nrs_surface_extract_aniso(m_ctx, &L, iso, flags, cfg, &V, &T) != NRS_OK) fatal("nrs_surface_extract_aniso");
    m_surfaceV = (SUint)V;
    m_surfaceT = (SUint)T;
}

// ---- diffuse particles -----------------------------------------------------------------------------------------------------------------
void SPH::configureDiffuse(const nrs_diffuse_config &cfg)
{
    ensureContext();
    nrs_diffuse_config c = cfg;
    c.struct_size = (uint32_t)sizeof(c);
    c.reserved = 0;
    if (nrs_diffuse_configure(m_ctx, &c) != NRS_OK) fatal("nrs_diffuse_configure");
}
void SPH::stepDiffuse(double dt)
{
    ensureContext();
    pushHostToDevice();
    if (nrs_diffuse_step(m_ctx, dt) != NRS_OK) fatal("nrs_diffuse_step");
}
template <typename T> static void fetchDiffuse(nrs_ctx *ctx, SUint which, std::vector<T> &v, bool &ok)
{
    uint64_t bytes = 0;
    ok = nrs_diffuse_result(ctx, which, nullptr, 0, &bytes) == NRS_OK;
    if (!ok) return;
    v.resize((size_t)(bytes / sizeof(T)));
    if (bytes) ok = nrs_diffuse_result(ctx, which, v.data(), bytes, nullptr) == NRS_OK;
}
SUint SPH::getDiffuse(const SVec4 **positions, const SVec4 **velocities, const SUint **kinds)
{
    bool ok = false;
    ensureContext();
    fetchDiffuse(m_ctx, NRS_DIFFUSE_POS, m_diffusePositions, ok);
    if (ok) fetchDiffuse(m_ctx, NRS_DIFFUSE_VEL, m_diffuseVelocities, ok);
    if (ok) fetchDiffuse(m_ctx, NRS_DIFFUSE_KIND, m_diffuseKinds, ok);
    if (!ok || m_diffuseVelocities.size() != m_diffusePositions.size() || m_diffuseKinds.size() != m_diffusePositions.size()) fatal("nrs_diffuse_result");
    if (positions) *positions = m_diffusePositions.data();
    if (velocities) *velocities = m_diffuseVelocities.data();
    if (kinds) *kinds = m_diffuseKinds.data();
    return (SUint)m_diffusePositions.size();
}

// ---- sources and sinks -------------------------------------------------------------------------------------------------------------------
void SPH::adoptDeviceCount()
{
    const SUint n = (SUint)nrs_num_particles(m_ctx);
    growHost(n);
    m_numParticles = n;
    m_deviceNewer = true;
    m_frameIsCurrent = false;
}
void SPH::setEmitter(SUint slot, const nrs_emitter *emitter)
{
    ensureContext();
    if (nrs_emitter_set(m_ctx, slot, emitter) != NRS_OK) fatal("nrs_emitter_set");
    m_inflow = true;
}
void SPH::getEmitter(SUint slot, nrs_emitter *emitter, unsigned long long *emitted, unsigned long long *dropped)
{
    ensureContext();
    uint64_t a = 0, d = 0;
    if (nrs_emitter_get(m_ctx, slot, emitter, &a, &d) != NRS_OK) fatal("nrs_emitter_get");
    if (emitted) *emitted = a;
    if (dropped) *dropped = d;
}
SUint SPH::emitBlock(const double origin[3], const double spacing[3], const SUint dims[3], const double vel[3])
{
    ensureContext();
    pushHostToDevice();
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.spacing[a] = spacing[a]; L.dims[a] = dims[a]; }
    uint64_t added = 0;
    const int rc = nrs_emit_block(m_ctx, &L, vel, &added);
    if (rc == NRS_E_CAPACITY) return 0;
    if (rc != NRS_OK) fatal("nrs_emit_block");
    adoptDeviceCount();
    return (SUint)added;
}
SUint SPH::emitMesh(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, const double origin[3], const double spacing[3],
                    const SUint dims[3], double clearance, const double vel[3])
{
    ensureContext();
    pushHostToDevice();
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.spacing[a] = spacing[a]; L.dims[a] = dims[a]; }
    const nrs_mesh mesh = {vertices.data(), (uint64_t)(vertices.size() / 3), triangles.data(), (uint64_t)(triangles.size() / 3)};
    const nrs_mesh_rule rule = {NRS_MESH_INSIDE, 0u, clearance, INFINITY};
    uint64_t added = 0;
    const int rc = nrs_emit_mesh(m_ctx, &mesh, &L, &rule, vel, &added);
    if (rc == NRS_E_CAPACITY) return 0;
    if (rc != NRS_OK) fatal("nrs_emit_mesh");
    adoptDeviceCount();
    return (SUint)added;
}
void SPH::setSinks(const nrs_sink_config *sinks)
{
    ensureContext();
    if (nrs_sinks_set(m_ctx, sinks) != NRS_OK) fatal("nrs_sinks_set");
    m_inflow = true;
}
SUint SPH::cull()
{
    ensureContext();
    pushHostToDevice();
    uint64_t removed = 0;
    if (nrs_cull(m_ctx, &removed) != NRS_OK) fatal("nrs_cull");
    if (removed) adoptDeviceCount();
    return (SUint)removed;
}
void SPH::sinkCounts(unsigned long long *removedTotal, unsigned long long *culls)
{
    ensureContext();
    uint64_t r = 0, c = 0;
    if (nrs_sinks_count(m_ctx, &r, &c) != NRS_OK) fatal("nrs_sinks_count");
    if (removedTotal) *removedTotal = r;
    if (culls) *culls = c;
}

nrs_ctx *SPH::deviceContext()
{
    ensureContext();
    return m_ctx;
}

void SPH::pushHostToDevice()
{
    if (m_hostDirty) {
        // a tracking context keeps identities: slots below the device's count are the same particles, rewritten; the rest are new
        const bool keep = m_tracking && !m_trackPending;
        const SUint onDevice = keep ? (SUint)nrs_num_particles(m_ctx) : 0;
        if ((!keep || onDevice > m_numParticles) && nrs_set_num_particles(m_ctx, keep ? m_numParticles : 0) != NRS_OK) fatal("nrs_set_num_particles");
        if (m_numParticles &&
            nrs_upload_particles(m_ctx, m_pos, m_vel, m_pressure, 0, m_numParticles) != NRS_OK)
            fatal("nrs_upload_particles");
        m_hostDirty = false;
        m_deviceNewer = false;
        m_colDirty = keep; // (the host's colours go with the host's particles)
    }
    if (!m_tracking) return;
    if (m_trackPending) {
        trackStart();
    } else if (m_colDirty) {
        if (m_numParticles && nrs_track_upload(m_ctx, NRS_TRACK_ATTRIBUTE, m_colors, 0, m_numParticles) != NRS_OK) fatal("nrs_track_upload");
        m_colDirty = false;
    }
}

// ---- particle tracking ---------------------------------------------------------------------------------------------------------------------
// the device's ids, births and colours into the host arrays, in the order of its positions
void SPH::fetchTracked() const
{
    const size_t n = (size_t)nrs_num_particles(m_ctx);
    m_ids.resize(n);
    m_birth.resize(n);
    if (!n) return;
    if (nrs_track_result(m_ctx, NRS_TRACK_ID, m_ids.data(), 4 * n, nullptr) != NRS_OK) fatal("nrs_track_result");
    if (nrs_track_result(m_ctx, NRS_TRACK_BIRTH, m_birth.data(), 4 * n, nullptr) != NRS_OK) fatal("nrs_track_result");
    if (n <= m_hostCapacity && nrs_track_result(m_ctx, NRS_TRACK_ATTRIBUTE, m_colors, sizeof(SReal) * 4 * n, nullptr) != NRS_OK) fatal("nrs_track_result");
}
// before a context is released to grow: what identifies its particles (the colours are on the host already, pullDeviceToHost)
void SPH::trackSave()
{
    if (!m_tracking || !m_ctx || m_trackPending) return;
    const size_t n = (size_t)nrs_num_particles(m_ctx);
    m_ids.resize(n);
    m_birth.resize(n);
    if (n && nrs_track_result(m_ctx, NRS_TRACK_ID, m_ids.data(), 4 * n, nullptr) != NRS_OK) fatal("nrs_track_result");
    if (n && nrs_track_result(m_ctx, NRS_TRACK_BIRTH, m_birth.data(), 4 * n, nullptr) != NRS_OK) fatal("nrs_track_result");
    uint64_t next = 0;
    if (nrs_track_info(m_ctx, nullptr, nullptr, &next) != NRS_OK) fatal("nrs_track_info");
    m_savedNextId = next;
    m_haveSaved = true;
}
// behind the first upload into a context: enable, put back what a released context had, the colours as the record, the emit colours
void SPH::trackStart()
{
    if (nrs_track_enable(m_ctx, NRS_TRACK_ATTR) != NRS_OK) fatal("nrs_track_enable");
    const size_t n = m_numParticles;
    if (m_haveSaved && n) {
        const size_t k = std::min(m_ids.size(), n);
        std::vector<SUint> ids(n), birth(n, 0);
        for (size_t i = 0; i < n; ++i) ids[i] = i < k ? m_ids[i] : (SUint)(m_savedNextId + (i - k)); // (particles the old context never saw)
        for (size_t i = 0; i < k; ++i) birth[i] = m_birth[i];
        if (m_savedNextId) { // ids are never reused: the counter passes the old one even where the largest ids have left (slot 0 is rewritten below)
            const SUint top = (SUint)(m_savedNextId - 1);
            if (nrs_track_upload(m_ctx, NRS_TRACK_ID, &top, 0, 1) != NRS_OK) fatal("nrs_track_upload");
        }
        if (nrs_track_upload(m_ctx, NRS_TRACK_ID, ids.data(), 0, n) != NRS_OK) fatal("nrs_track_upload");
        if (nrs_track_upload(m_ctx, NRS_TRACK_BIRTH, birth.data(), 0, n) != NRS_OK) fatal("nrs_track_upload");
    }
    m_haveSaved = false;
    if (n && nrs_track_upload(m_ctx, NRS_TRACK_ATTRIBUTE, m_colors, 0, n) != NRS_OK) fatal("nrs_track_upload");
    for (int s = 0; s < 17; ++s)
        if (m_emitColorSet[s] && nrs_track_emit_value(m_ctx, s - 1, m_emitColors[s]) != NRS_OK) fatal("nrs_track_emit_value");
    m_trackPending = false;
    m_colDirty = false;
    m_ids.clear();
    m_birth.clear();
}
void SPH::setParticleTracking(bool on)
{
    if (on == m_tracking) return;
    if (on) {
        m_tracking = true;
        m_trackPending = true;
        if (m_ctx) pushHostToDevice();
        return;
    }
    if (m_ctx && !m_trackPending) {
        pullDeviceToHost(); // (the colours stay as the device had them)
        if (nrs_track_disable(m_ctx) != NRS_OK) fatal("nrs_track_disable");
    }
    m_tracking = m_trackPending = m_colDirty = m_haveSaved = false;
}
const SUint *SPH::getHostIds()
{
    if (!m_tracking) return nullptr;
    ensureContext();
    pushHostToDevice();
    pullDeviceToHost();
    if (m_ids.size() != m_numParticles) fetchTracked();
    return m_ids.data();
}
const SUint *SPH::getHostBirth()
{
    if (!getHostIds()) return nullptr;
    return m_birth.data();
}
void SPH::setEmitterColor(int slot, SVec4 c)
{
    if (slot < -1 || slot > 15) { std::fprintf(stderr, "Nereus: setEmitterColor: slot must be -1 .. 15\n"); std::exit(EXIT_FAILURE); }
    const double a[4] = {(double)c.x, (double)c.y, (double)c.z, (double)c.w};
    std::memcpy(m_emitColors[slot + 1], a, sizeof(a));
    m_emitColorSet[slot + 1] = true;
    if (m_tracking && m_ctx && !m_trackPending && nrs_track_emit_value(m_ctx, slot, a) != NRS_OK) fatal("nrs_track_emit_value");
}
void SPH::diffuseColors(const double kappa[4], double dt)
{
    if (!m_tracking) { std::fprintf(stderr, "Nereus: diffuseColors needs setParticleTracking(true)\n"); std::exit(EXIT_FAILURE); }
    ensureContext();
    pushHostToDevice();
    if (nrs_track_diffuse(m_ctx, kappa, dt) != NRS_OK) fatal("nrs_track_diffuse");
    m_deviceNewer = true; // (the colours on the device are newer than the host's)
    m_ids.clear();
}
const std::vector<SUint> &SPH::locateParticles(unsigned long long first, SUint count)
{
    if (!m_tracking) { std::fprintf(stderr, "Nereus: locateParticles needs setParticleTracking(true)\n"); std::exit(EXIT_FAILURE); }
    ensureContext();
    pushHostToDevice();
    if (nrs_track_locate(m_ctx, first, count) != NRS_OK) fatal("nrs_track_locate");
    m_slotOf.resize(count);
    if (count && nrs_track_result(m_ctx, NRS_TRACK_SLOT_OF, m_slotOf.data(), 4 * (uint64_t)count, nullptr) != NRS_OK) fatal("nrs_track_result");
    return m_slotOf;
}

void SPH::pullDeviceToHost() const
{
    if (!m_deviceNewer || !m_ctx) return;
    const bool wantPressure = solverKind() == NRS_SOLVER_IISPH || solverKind() == NRS_SOLVER_PCISPH || solverKind() == NRS_SOLVER_PBF ||
                              solverKind() == NRS_SOLVER_DFSPH;
    if (nrs_download(m_ctx, m_pos, m_vel, wantPressure ? m_pressure : nullptr) != NRS_OK) fatal("nrs_download");
    if (m_tracking && !m_trackPending) fetchTracked(); // the colours, ids and births of the same order
    m_deviceNewer = false;
}

void SPH::synchronize() const
{
    if (m_ctx && nrs_synchronize(m_ctx) != NRS_OK) fatal("nrs_synchronize");
}

void SPH::update()
{
    if (m_numParticles == 0 && !m_inflow) return; // (an emitter steps from empty)
    ensureContext();
    pushHostToDevice();                                                   // only if the host side changed
    if (m_cfl) { // sph.cpp:217-231 (disabled there): newDeltat = lambda * (ir / |v|max)
        double vmax = 0.0;
        if (nrs_max_velocity(m_ctx, &vmax) != NRS_OK) fatal("nrs_max_velocity");
        if (vmax > 0.0) m_params.timestep = m_cflLambda * (m_params.interactionRadius / (SReal)vmax);
    }
    if (nrs_set_params(m_ctx, &m_params) != NRS_OK) fatal("nrs_set_params"); // setParameters, every step
    if (nrs_step(m_ctx, 1) != NRS_OK) fatal("nrs_step");
    m_deviceNewer = true;
    m_frameIsCurrent = false;
    if (m_inflow) adoptDeviceCount(); // sources and sinks: the count is the device's
    if (m_asyncReadback) {
        if (m_framesInFlight == 2) collectFrames(false); // the library would wait for the oldest anyway: keep it
        if (nrs_snapshot_begin(m_ctx, 0) != NRS_OK) fatal("nrs_snapshot_begin");
        ++m_framesInFlight;
    }
    if (m_eagerSync) pullDeviceToHost();
}

void SPH::setAsyncReadback(bool on)
{
    if (!on && m_ctx) collectFrames(true);
    m_asyncReadback = on;
}

// take every finished snapshot out of the library (all of them, blocking, if waitForAll; else at least the oldest when
// two are in flight or none has ever arrived)
void SPH::collectFrames(bool waitForAll) const
{
    while (m_framesInFlight > 0) {
        const bool mustWait = waitForAll || m_framesInFlight == 2 || m_frame == nullptr;
        const void *p = nullptr;
        uint64_t n = 0, step = 0;
        const int rc = nrs_snapshot_wait(m_ctx, mustWait ? 1 : 0, &p, nullptr, &n, &step);
        if (rc == NRS_E_NOTREADY) break;
        if (rc != NRS_OK) fatal("nrs_snapshot_wait");
        --m_framesInFlight;
        m_frame = (const SReal *)p;
        m_frameCount = (SUint)n;
        m_frameStep = step;
        m_frameIsCurrent = (m_framesInFlight == 0); // the newest begun snapshot was taken right after the last update()
    }
}

const SReal *SPH::latestFrame(SUint *numParticles, unsigned long long *step)
{
    if (!m_asyncReadback || !m_ctx) { // no snapshots: the synchronous path
        pullDeviceToHost();
        if (numParticles) *numParticles = m_numParticles;
        if (step) *step = 0;
        return m_pos;
    }
    collectFrames(false);
    if (numParticles) *numParticles = m_frameCount;
    if (step) *step = m_frameStep;
    return m_frame;
}

SReal *&SPH::getPos() { pullDeviceToHost(); m_hostDirty = true; return m_pos; }
SReal *&SPH::getVel() { pullDeviceToHost(); m_hostDirty = true; return m_vel; }
SReal *&SPH::getCol()
{
    if (m_tracking) { // the colours in the order of the positions; the caller may write them
        if (m_ctx && !m_trackPending) pullDeviceToHost();
        m_colDirty = true;
    }
    return m_colors;
}
SReal *SPH::getHostPos() const
{
    if (m_asyncReadback && m_ctx && m_deviceNewer && m_framesInFlight > 0) collectFrames(true);
    if (m_asyncReadback && m_frameIsCurrent && m_deviceNewer && m_frame) return const_cast<SReal *>(m_frame);
    pullDeviceToHost();
    return m_pos;
}
SReal *SPH::getHostVel() const { pullDeviceToHost(); return m_vel; }
SReal *SPH::getHostPressure() const { pullDeviceToHost(); return m_pressure; }
SReal *SPH::getHostCol() const
{
    if (m_tracking && m_ctx && !m_trackPending) pullDeviceToHost(); // tracking: in the order of getHostPos(); else as the caller filled it
    return m_colors;
}

std::pair<SVec3, SVec3> SPH::computeGridMinMax() const
{
    // BBMin/BBMax of the reference run three reductions per bound on the device copy; the values are the
    // per-axis extrema of the boundary positions, computed here on the caller's array.
    SVec3 lo = make_SVec3(0, 0, 0), hi = make_SVec3(0, 0, 0);
    if (m_bi && m_num_boundaries) {
        lo = hi = make_SVec3(m_bi[0], m_bi[1], m_bi[2]);
        for (SUint i = 1; i < m_num_boundaries; ++i) {
            const SReal *q = m_bi + 4 * (size_t)i;
            if (q[0] < lo.x) lo.x = q[0];
            if (q[1] < lo.y) lo.y = q[1];
            if (q[2] < lo.z) lo.z = q[2];
            if (hi.x < q[0]) hi.x = q[0];
            if (hi.y < q[1]) hi.y = q[1];
            if (hi.z < q[2]) hi.z = q[2];
        }
    }
    return std::make_pair(lo, hi);
}

void SPH::updateGrid()
{
    const std::pair<SVec3, SVec3> bb = computeGridMinMax();
    m_params.worldOrigin = make_SVec3(bb.first.x - 0.1, bb.first.y - 0.1, bb.first.z - 0.1);
    const SUint nx = std::ceil((bb.second.x - bb.first.x + 0.1) / m_params.interactionRadius);
    const SUint ny = std::ceil((bb.second.y - bb.first.y + 0.1) / m_params.interactionRadius);
    const SUint nz = std::ceil((bb.second.z - bb.first.z + 0.1) / m_params.interactionRadius);
    m_params.gridSize = make_uint3(nextPow2(nx), nextPow2(ny), nextPow2(nz));
    m_params.numCells = m_params.gridSize.x * m_params.gridSize.y * m_params.gridSize.z;
    _initializeGrid();
    if (m_ctx && nrs_set_params(m_ctx, &m_params) != NRS_OK) fatal("nrs_set_params");
}

void SPH::addNewParticle(SVec4 p, SVec4 v)
{
    pullDeviceToHost(); // appending to stale host arrays would lose the device state
    if (m_numParticles >= m_hostCapacity) growHost(std::max<SUint>(2 * m_hostCapacity, 1024));
    const size_t i = m_numParticles;
    m_pos[4 * i + 0] = p.x; m_pos[4 * i + 1] = p.y; m_pos[4 * i + 2] = p.z; m_pos[4 * i + 3] = p.w;
    m_vel[4 * i + 0] = v.x; m_vel[4 * i + 1] = v.y; m_vel[4 * i + 2] = v.z; m_vel[4 * i + 3] = v.w;
    m_density[i] = 0.0;
    m_pressure[i] = 0.0;
    for (int c = 0; c < 4; ++c) m_forces[4 * i + c] = 0.0;
    m_colors[4 * i + 0] = 1.0; m_colors[4 * i + 1] = 0.0; m_colors[4 * i + 2] = 0.0; m_colors[4 * i + 3] = 1.0;
    m_numParticles += 1;
    m_hostDirty = true;
}

void SPH::generateParticleCube(SVec4 center, SVec4 size, SVec4 vel)
{
    const SReal step = m_params.interactionRadius - 0.005f;
    for (SReal x = center.x - size.x / 2.0; x <= center.x + size.x / 2.0; x += step)
        for (SReal y = center.y - size.y / 2.0; y <= center.y + size.y / 2.0; y += step)
            for (SReal z = center.z - size.z / 2.0; z <= center.z + size.z / 2.0; z += step)
                addNewParticle(make_SVec4(x, y, z, 1.0), vel);
    std::cout << "There were " << m_numParticles << " particles generated." << std::endl;
}

namespace {
struct CkptHeader {
    char magic[8];
    uint32_t realBytes, solver, paramBytes, reserved;
    uint64_t n;
};
} // namespace

bool SPH::saveState(const char *path) const
{
    pullDeviceToHost();
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    CkptHeader h;
    std::memcpy(h.magic, "NRSCKPT1", 8);
    h.realBytes = sizeof(SReal); h.solver = (uint32_t)solverKind(); h.paramBytes = sizeof(SphSimParams); h.reserved = 0;
    h.n = m_numParticles;
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1 && std::fwrite(&m_params, sizeof(m_params), 1, f) == 1;
    const size_t n = m_numParticles;
    ok = ok && (n == 0 || (std::fwrite(m_pos, sizeof(SReal) * 4, n, f) == n && std::fwrite(m_vel, sizeof(SReal) * 4, n, f) == n &&
                           std::fwrite(m_pressure, sizeof(SReal), n, f) == n));
    return std::fclose(f) == 0 && ok;
}

bool SPH::loadState(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    CkptHeader h;
    bool ok = std::fread(&h, sizeof(h), 1, f) == 1 && std::memcmp(h.magic, "NRSCKPT1", 8) == 0 && h.realBytes == sizeof(SReal) &&
              h.paramBytes == sizeof(SphSimParams) && h.solver == (uint32_t)solverKind() && h.n < (1ull << 27);
    SphSimParams p;
    ok = ok && std::fread(&p, sizeof(p), 1, f) == 1;
    if (ok) {
        const size_t n = (size_t)h.n;
        growHost((SUint)std::max<size_t>(n, 1));
        ok = n == 0 || (std::fread(m_pos, sizeof(SReal) * 4, n, f) == n && std::fread(m_vel, sizeof(SReal) * 4, n, f) == n &&
                        std::fread(m_pressure, sizeof(SReal), n, f) == n);
        if (ok) {
            // keep the grid of the running solver if boundaries already fixed it; take everything else from the file
            m_params = p;
            m_numParticles = (SUint)n;
            m_hostDirty = true;
            m_deviceNewer = false;
        }
    }
    std::fclose(f);
    return ok;
}

void SPH::updateGpuBoundaries(SUint nb_boundary_spheres)
{
    m_num_boundaries = nb_boundary_spheres ? nb_boundary_spheres : m_num_boundaries;
    if (!m_bi || !m_vbi || !m_num_boundaries) {
        std::fprintf(stderr, "Nereus: updateGpuBoundaries called without setBi/setVbi/setNumBoundaries\n");
        std::exit(EXIT_FAILURE);
    }
    ensureContext();
    // grid from the boundary AABB (updateGrid), then hash / sort / cell ranges of the boundary particles
    if (nrs_set_params(m_ctx, &m_params) != NRS_OK) fatal("nrs_set_params");
    if (nrs_set_boundaries(m_ctx, m_bi, m_vbi, m_num_boundaries, 1) != NRS_OK) fatal("nrs_set_boundaries");
    m_bodyOf.clear(); // (nrs_set_boundaries clears the body assignment)
    m_numBodies = 0;
    if (nrs_get_params(m_ctx, &m_params) != NRS_OK) fatal("nrs_get_params");
    m_boundariesPending = false;
    std::cout << "boundaries updated !" << std::endl;
}

NEREUS_NAMESPACE_END
