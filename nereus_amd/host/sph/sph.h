// sph.h — Nereus::SPH, the state-equation SPH (SESPH) solver, MI355X build.
//
// Public surface = the reference's sph/sph.h:26-94 (same method names, argument meaning and error behaviour),
// so main.cpp and other callers compile unchanged.  Everything below the API is new: the particle state
// lives on the GPU inside an nrs_ctx (include/nereus_hip.h); host arrays are synchronised on demand.
#pragma once
#ifndef SPH_H
#define SPH_H

#include <cstdint>
#include <utility>
#include <vector>

#if defined(__has_include)
#if __has_include(<glm/glm.hpp>)
#ifndef GLM_SWIZZLE
#define GLM_SWIZZLE
#endif
#include <glm/glm.hpp> // optional: no GLM type appears in this API
#endif
#endif

#include "common.h"
#include "sph_kernel.cuh"
#include <colored_output.h>

// Initial particle capacity.  The reference hard-caps at this number (sph/sph.h:19); here it is only the
// starting size: host and device storage grow on demand (or set NEREUS_CAPACITY / call reserveParticles()).
#define MAX_PARTICLE_NUMBER 150000

struct nrs_ctx;
struct nrs_aniso_config;
struct nrs_diffuse_config;
struct nrs_emitter;
struct nrs_sink_config;

NEREUS_NAMESPACE_BEGIN

class SPH {
public:
    SPH();
    SPH(SphSimParams params);
    virtual ~SPH();

    // life cycle (idempotent: may be called again, as main.cpp:534 does)
    virtual void _initialize();
    virtual void _finalize();
    virtual void _initializeGrid();

    // fluid creation; particles may be appended between steps (main.cpp:499-513)
    virtual void addNewParticle(SVec4 p, SVec4 v);
    virtual void generateParticleCube(SVec4 center, SVec4 size, SVec4 vel);

    // one simulation step; on return the new state is observable through the getters
    virtual void update();

    // grid sizing from the boundary AABB
    void updateGrid();
    std::pair<SVec3, SVec3> computeGridMinMax() const;

    // physics constants
    SReal getGasStiffness() const { return m_params.gasStiffness; }
    SReal getRestDensity() const { return m_params.restDensity; }
    SReal getParticleMass() const { return m_params.particleMass; }
    SReal getParticleRadius() const { return m_params.particleRadius; }
    SReal getTimestep() const { return m_params.timestep; }
    SReal getViscosity() const { return m_params.viscosity; }
    SReal getSurfaceTension() const { return m_params.surfaceTension; }
    SReal getInteractionRadius() const { return m_params.interactionRadius; }
    SUint getNumCells() const { return m_params.numCells; }
    void setGasStiffness(SReal v) { m_params.gasStiffness = v; }
    void setRestDensity(SReal v) { m_params.restDensity = v; }
    void setParticleMass(SReal v) { m_params.particleMass = v; }
    void setViscosity(SReal v) { m_params.viscosity = v; }
    void setSurfaceTension(SReal v) { m_params.surfaceTension = v; }
    void setGravity(SReal gy) { m_params.gravity.y = gy; }

    // particle arrays, AoS xyzw, 4*getNumParticles() SReals, owned by the solver, valid until the next
    // update()/append/destruction.  The mutable accessors assume the caller may write and re-upload the
    // arrays before the next step; the const ones only read.
    SReal *&getPos();
    SReal *&getCol();
    SReal *&getVel();
    SReal *getHostPos() const;
    SReal *getHostCol() const;
    SUint getNumParticles() const { return m_numParticles; }

    // boundary particles: caller keeps ownership of bi (xyzw) / vbi; copied in updateGpuBoundaries
    void setBi(SReal *bi) { m_bi = bi; }
    void setVbi(SReal *vbi) { m_vbi = vbi; }
    void setNumBoundaries(SUint nb) { m_num_boundaries = nb; }
    void updateGpuBoundaries(SUint nb_boundary_spheres);

    // ---- additions of this build (not in the reference) ----
    // Kinematic boundary bodies (nrs_set_boundary_bodies and friends, DESIGN.md "Kinematic boundary bodies"), after
    // updateGpuBoundaries: bodyOf[i] in 0 .. nbodies-1 per boundary particle, body 0 the static world; the context moves bodies
    // 1 .. nbodies-1 every update() and rebuilds the boundary tables on the device.  A later updateGpuBoundaries clears the assignment.
    // The assignment is kept and applied again when the device context is rebuilt (capacity growth), the poses then restart at rest;
    // saveState / loadState do not hold poses.  Errors end the program, as every device error of this class does.
    void setBoundaryBodies(const SUint *bodyOf, SUint nbodies);
    void setBodyVelocity(SUint body, const double v[3], const double omega[3]);
    void setBodyPose(SUint body, const double x[3], const double q[4]);
    void getBodyPose(SUint body, double x[3], double q[4]);
    // Field sampling (nrs_sample_*, DESIGN.md "Field sampling"): the SPH fields of the current state — density, its gradient, the
    // Shepard-averaged velocity, the neighbour count (NRS_FIELD_* flags in `fields`, NRS_FIELD_WALLS adds the wall term to the density)
    // — at n points, or on the dims[0] x dims[1] x dims[2] nodes origin + idx * spacing (node (i, j, k) at (k * dims[1] + j) * dims[0] + i).
    // Both enqueue and return; the getters wait and return the field of the LAST sample call in a host array the solver owns, valid
    // until the next getter call for that field.  Read-only: the simulation does not notice.
    void sampleLattice(const double origin[3], const double spacing[3], const SUint dims[3], SUint fields);
    void samplePoints(const SVec4 *points, SUint n, SUint fields);
    const std::vector<SReal> &getSampledDensity();
    const std::vector<SVec4> &getSampledGradient();
    const std::vector<SVec4> &getSampledVelocity();
    const std::vector<SUint> &getSampledCount();
    // Surface extraction (nrs_surface_*, DESIGN.md "Surface extraction"): the iso-surface density = iso of the current state as an
    // indexed triangle mesh, by marching tetrahedra on the lattice, on the device.  It IS sampleLattice (density, plus what the
    // NRS_SURFACE_* flags ask for) followed by the mesher, so getSampledDensity() afterwards is the lattice the mesh was cut from.  Waits
    // for the device once (the totals size the outputs).  The getters return one result of the LAST extract in a host array the solver
    // owns: vertices (x, y, z, t), three vertex numbers per triangle, and the per-vertex gradient / velocity if asked for.
    void extractSurface(const double origin[3], const double spacing[3], const SUint dims[3], double iso, SUint flags);
    SUint getSurfaceNumVertices() const { return m_surfaceV; }
    SUint getSurfaceNumTriangles() const { return m_surfaceT; }
    const std::vector<SVec4> &getSurfaceVertices();
    const std::vector<SUint> &getSurfaceTriangles();
    const std::vector<SVec4> &getSurfaceGradient();
    const std::vector<SVec4> &getSurfaceVelocity();
    // Anisotropic surface reconstruction (nrs_aniso_* / nrs_surface_extract_aniso, DESIGN.md "Anisotropic kernels"; Yu & Turk 2013).
    // anisoKernels builds one ellipsoidal kernel per fluid particle, in the sampler's sorted order (cfg null: the library's defaults), and
    // returns without waiting; the getters wait and return one result of the LAST build in a host array the solver owns: centre + largest
    // semi-axis; two SVec4 per particle (G00, G01, G02, G11), (G12, G22, weight, 0); the neighbour count; the particle's index in host order.
    // extractSurfaceAniso builds the kernels, evaluates their colour field phi on the lattice INTO the sampled fields (getSampledDensity()
    // afterwards is phi, the lattice the mesh was cut from) and meshes phi = iso; the mesh comes back through the getSurface* getters.
    void anisoKernels(const nrs_aniso_config *cfg = nullptr);
    const std::vector<SVec4> &getAnisoCenters();
    const std::vector<SVec4> &getAnisoG();
    const std::vector<SUint> &getAnisoCount();
    const std::vector<SUint> &getAnisoIndex();
    void extractSurfaceAniso(const double origin[3], const double spacing[3], const SUint dims[3], double iso, SUint flags,
                             const nrs_aniso_config *cfg = nullptr);
    // Diffuse particles (nrs_diffuse_*, DESIGN.md "Diffuse particles"): spray, foam and bubbles born from the fluid's trapped air, wave
    // crests and kinetic energy, kept and advected on the device.  configureDiffuse stores the configuration (struct_size and reserved are
    // filled in); stepDiffuse advances the set on the current state (dt 0: the timestep) and returns without waiting — call it after
    // update(); getDiffuse waits and returns the living set in host arrays the solver owns (positions with the remaining lifetime in w,
    // velocities, kinds 0 spray / 1 foam / 2 bubble), valid until the next call.  Read-only: the simulation does not notice.
    void configureDiffuse(const nrs_diffuse_config &cfg);
    void stepDiffuse(double dt = 0.0);
    SUint getDiffuse(const SVec4 **positions, const SVec4 **velocities, const SUint **kinds);
    // Sources and sinks (nrs_emitter_* / nrs_sinks_* / nrs_cull / nrs_emit_block, DESIGN.md "Sources and sinks"): emitters append layers of
    // particles at the top of every update(), kill volumes remove particles there, all on the device; update() then also runs on an empty
    // solver, and getNumParticles() follows the device's count.  setEmitter(slot, nullptr) removes a slot, setSinks(nullptr) clears the
    // sinks.  emitBlock appends the nodes of a lattice with one velocity and returns their number, 0 when they do not fit the capacity
    // (reserveParticles first); cull runs one cull now and returns the number removed.  The device context holds the configuration:
    // reserve the capacity BEFORE configuring (a context rebuilt to grow starts without emitters and sinks), and saveState / loadState
    // do not hold emitters, sinks, accumulators or counts.
    void setEmitter(SUint slot, const nrs_emitter *emitter);
    void getEmitter(SUint slot, nrs_emitter *emitter, unsigned long long *emitted, unsigned long long *dropped);
    SUint emitBlock(const double origin[3], const double spacing[3], const SUint dims[3], const double vel[3]);
    // emitMesh: emitBlock restricted to the nodes inside a triangle mesh (vertices: 3 doubles each; triangles: 3 indices each, wound
    // counter-clockwise seen from outside) and at least `clearance` away from it (nrs_emit_mesh with NRS_MESH_INSIDE, dmin = clearance,
    // dmax = infinity: "fill this shape with fluid"); sample_spheres::ss::meshLattice gives the lattice that walls sampled from meshes use.
    SUint emitMesh(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, const double origin[3], const double spacing[3],
                   const SUint dims[3], double clearance, const double vel[3]);
    void setSinks(const nrs_sink_config *sinks);
    SUint cull();
    void sinkCounts(unsigned long long *removedTotal, unsigned long long *culls);
    // Particle tracking (nrs_track_*, DESIGN.md "Particle identity and attributes"), off by default; while it is off the colours behave
    // as in the reference: getHostCol() is the array as the caller filled it, never permuted.  While it is on, the device context is
    // enabled with NRS_TRACK_ATTR and the colours travel as the attribute record: getHostCol() / getCol() return them in the order of
    // getHostPos(), getHostIds() and getHostBirth() give each particle's id (unique for the life of the solver, also across a context
    // rebuilt to grow) and the update() count at its entry, in the same order.  Particles present when tracking starts are numbered
    // 0 .. n-1 in host order; rewriting positions through getPos() keeps identities, appended particles get new ids.
    // setEmitterColor(slot, c): the colour of emitter `slot`'s particles, slot -1 that of emitBlock's.  diffuseColors: one explicit
    // diffusion step of the colours between neighbours (nrs_track_diffuse; dt 0: the timestep; stable while 2 dt kappa restDensity
    // sum |w_ij| <= 1, not checked).  locateParticles(first, count): the index in getHostPos() order of ids first .. first + count - 1,
    // 0xffffffff for an id that is gone, in a host array the solver owns.  A context rebuilt to grow keeps ids, births and colours (the
    // class pulls them and puts them back with nrs_track_upload); emitter colours are applied again.
    void setParticleTracking(bool on);
    bool getParticleTracking() const { return m_tracking; }
    const SUint *getHostIds();
    const SUint *getHostBirth();
    void setEmitterColor(int slot, SVec4 color);
    void diffuseColors(const double kappa[4], double dt = 0.0);
    const std::vector<SUint> &locateParticles(unsigned long long first, SUint count);
    void reserveParticles(SUint capacity);        // grow host+device storage up front
    void setEagerSync(bool on) { m_eagerSync = on; } // true: D2H at the end of every update() like the reference
    const SphSimParams &getParams() const { return m_params; }
    SReal *getHostVel() const;
    SReal *getHostPressure() const;
    void synchronize() const;                       // wait for the device
    nrs_ctx *deviceContext();                      // the underlying C-ABI handle (created on demand)
    // CFL time step, the block the reference keeps under `#if 0` (sph/sph.cpp:217-231): before each step
    // dt = lambda * h / max|v| (lambda = 0.4) from a device-side reduction; off by default as in the reference build
    void setAdaptiveTimestep(bool on, SReal lambda = 0.4f) { m_cfl = on; m_cflLambda = lambda; }
    // binary checkpoint of the particle state (parameters, positions, velocities, IISPH warm-start pressure);
    // the reference has none.  A restored solver continues bit-identically.  The format does not hold particle ids, births
    // or colours: a solver that tracks its particles numbers a loaded state afresh, as it does not hold poses, emitters or sinks.
    bool saveState(const char *path) const;
    bool loadState(const char *path);
    // Viewer hand-off that does not stall the solver (the reference copies pos+vel back synchronously at the end of every
    // update(), sph.cpp:283-284, and main.cpp:587-588 uploads them to a VBO).  With asynchronous read-back on, update()
    // also starts a device -> page-locked-host copy of the new positions on a copy stream (nrs_snapshot_begin), which
    // overlaps with the updates enqueued after it.  latestFrame() never waits for the solver: it returns the newest
    // frame whose transfer has completed (at most two updates old; it blocks only while no frame has arrived yet);
    // getHostPos() keeps the reference's meaning (positions after the last update()) and waits for that frame.
    void setAsyncReadback(bool on);
    const SReal *latestFrame(SUint *numParticles = nullptr, unsigned long long *step = nullptr);

protected:
    virtual int solverKind() const; // NRS_SOLVER_*
    virtual void configureContext() {} // solver settings of a freshly created device context (ensureContext)
    void ensureContext();
    void releaseContext();
    void growHost(SUint capacity);
    void pushHostToDevice();
    void pullDeviceToHost() const;
    [[noreturn]] void fatal(const char *what) const;

    SphSimParams m_params;
    SUint m_gridSortBits; // kept: the reference sets 32 and never uses it

    // host arrays (m_pos etc. keep the reference's names for derived classes)
    mutable SReal *m_pos, *m_vel, *m_density, *m_pressure, *m_forces, *m_colors;
    SUint m_numParticles;
    SUint m_hostCapacity;

    SReal *m_bi, *m_vbi; // caller-owned
    SUint m_num_boundaries;

    // device side
    nrs_ctx *m_ctx;
    SUint m_ctxCapacity;
    bool m_hostDirty;           // host arrays changed since the last upload
    mutable bool m_deviceNewer; // device holds a newer state than the host arrays
    bool m_boundariesPending;   // boundaries known but not yet uploaded into (a new) context
    std::vector<SUint> m_bodyOf; // boundary body assignment (empty: none), re-applied to a new context
    SUint m_numBodies;
    bool m_eagerSync;
    bool m_initialized;
    bool m_cfl;
    SReal m_cflLambda;
    bool m_asyncReadback;
    mutable int m_framesInFlight;        // snapshots begun and not yet collected (0..2)
    mutable const SReal *m_frame;        // newest collected frame (library-owned pinned memory)
    mutable SUint m_frameCount;
    mutable unsigned long long m_frameStep;
    mutable bool m_frameIsCurrent;       // m_frame shows the state after the last update()
    void collectFrames(bool waitForAll) const;
    std::vector<SReal> m_sampledDensity; // host copies of the last sample call's results, fetched by the getters
    std::vector<SVec4> m_sampledGradient, m_sampledVelocity;
    std::vector<SUint> m_sampledCount;
    std::vector<SVec4> m_surfaceVertices, m_surfaceGradient, m_surfaceVelocity; // ... and of the last surface extract
    std::vector<SUint> m_surfaceTriangles;
    SUint m_surfaceV = 0, m_surfaceT = 0;
    std::vector<SVec4> m_anisoCenters, m_anisoG; // host copies of the results of the last anisoKernels
    std::vector<SUint> m_anisoCount, m_anisoIndex;
    std::vector<SVec4> m_diffusePositions, m_diffuseVelocities; // ... and the living diffuse set of the last getDiffuse
    std::vector<SUint> m_diffuseKinds;
    bool m_inflow = false; // emitters or sinks were configured: the device's particle count leads
    void adoptDeviceCount();
    // particle tracking: asked for / the context still has to be enabled (trackStart, at the next upload) / colours edited on the host
    bool m_tracking = false, m_trackPending = false, m_colDirty = false;
    mutable std::vector<SUint> m_ids, m_birth; // host copies, in getHostPos() order
    std::vector<SUint> m_slotOf;               // the last locateParticles
    bool m_haveSaved = false;                  // m_ids / m_birth hold what a released context had: trackStart puts them back
    unsigned long long m_savedNextId = 0;
    double m_emitColors[17][4] = {};           // [slot + 1]
    bool m_emitColorSet[17] = {};
    void trackStart();
    void trackSave();
    void fetchTracked() const;
};

NEREUS_NAMESPACE_END
#endif // SPH_H
