/*
 * nereus_hip.h — C ABI of libnereus_hip.so: the MI355X (gfx950) SPH fluid step behind the host
 * classes Nereus::SPH / Nereus::IISPH.
 *
 * This is the boundary a host program binds (C, C++, ctypes, cgo, JNI ...): plain pointers and sizes,
 * no C++ or torch types.  It REPLACES the reference's CUDA launcher layer, the `extern "C"` block of
 * sph/sph.cuh:19-230 (defined in sph/sph_cuda.cu), with a context API (nrs_*): device-resident particle
 * state, one call per update().  It is what nereus_amd/host/ (our Nereus::SPH / Nereus::IISPH) and bench.py
 * use; INTEGRATION.md maps every reference entry point to its replacement.
 *
 * The library reads NO environment variables: every switch that changes which kernels run is an NRS_FLAG_* bit of nrs_config.flags.
 * Conventions: every nrs_* call returns 0 on success, a negative NRS_E_* code otherwise, and
 * nrs_last_error() gives the message (no exceptions cross the ABI).  The caller owns host buffers,
 * the library owns device buffers.  A context is bound to one HIP device and one stream; it is not
 * thread-safe.  Particle arrays are AoS xyzw of SReal exactly as the reference's host arrays
 * (sph/sph.cpp:341-368): pos4/vel4 = 4*N SReal, scalars = N SReal; SReal = float or double by
 * nrs_config.precision (the reference's DOUBLE_PRECISION switch, common/common.h:23-43).
 */
#ifndef NEREUS_HIP_H
#define NEREUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SphSimParams (common/sph_kernel.cuh:13-59), SReal=float: 132 bytes, align 4. */
typedef struct nrs_params_f32 {
    uint32_t gridSize[3];
    uint32_t numCells;
    float worldOrigin[3];
    float cellSize[3];
    uint32_t numBodies;
    uint32_t maxParticlesPerCell;
    float gasStiffness, viscosity, surfaceTension, restDensity, particleMass, interactionRadius, timestep,
        particleRadius;
    float gravity[3];
    float soundSpeed;
    float beta;
    float kpoly, kpoly_grad, kpress_grad, kvisc_grad, kvisc_denum, ksurf1, ksurf2, bpol;
} nrs_params_f32;

/* SphSimParams, SReal=double: 240 bytes, align 8. */
typedef struct nrs_params_f64 {
    uint32_t gridSize[3];
    uint32_t numCells;
    double worldOrigin[3];
    double cellSize[3];
    uint32_t numBodies;
    uint32_t maxParticlesPerCell;
    double gasStiffness, viscosity, surfaceTension, restDensity, particleMass, interactionRadius, timestep,
        particleRadius;
    double gravity[3];
    double soundSpeed;
    double beta;
    double kpoly, kpoly_grad, kpress_grad, kvisc_grad, kvisc_denum, ksurf1, ksurf2, bpol;
} nrs_params_f64;

typedef struct nrs_ctx nrs_ctx;

/* Nereus::SPH (sph/sph.h:23) / Nereus::IISPH (iisph.h:8) / predictive-corrective PCISPH (Solenthaler & Pajarola 2009; the
 * reference's Nereus::PCISPH stops after the density, its pressure solve is an empty stub: DESIGN.md "PCISPH" defines this one) /
 * position-based fluids (Macklin & Mueller 2013; DESIGN.md "PBF") / divergence-free SPH (Bender & Koschier 2015; DESIGN.md "DFSPH").
 * PBF and DFSPH came after nrs_version() 0.3 without a version change: a library supports one when nrs_create accepts its id. */
enum { NRS_SOLVER_SESPH = 0, NRS_SOLVER_IISPH = 1, NRS_SOLVER_PCISPH = 2, NRS_SOLVER_PBF = 3, NRS_SOLVER_DFSPH = 4 };
enum { NRS_KERNELS_MONAGHAN = 0, NRS_KERNELS_MULLER = 1 }; /* KERNEL_SET, common/common.h:14-15 */

/* nrs_config.flags */
enum {
    NRS_FLAG_REFERENCE_ORDER = 1u << 0, /* gather kernels walk the 27 cells and sum in exactly the reference's
                                           order (one thread per slot, per-cell partial sums): slower, used for
                                           bit-level comparison with the oracle */
    NRS_FLAG_NO_FUSION = 1u << 2,       /* keep forces, integrate and hash as three launches (default: a full step
                                           on the production kernels fuses them into the force kernel) */
    NRS_FLAG_NO_SHARED_LISTS = 1u << 3, /* the force kernel re-scans the neighbourhood instead of consuming the hit lists
                                           the density kernel of the same step found (saves HIT_CAP*4 B/particle of HBM) */
    NRS_FLAG_FULL_SORT = 1u << 4,       /* sort all (hash, index) pairs from scratch every step, as the reference does
                                           (sph_cuda.cu:310-313); default: only the particles that changed cell are
                                           sorted and merged into the still-sorted rest (same result, element for element) */
    NRS_FLAG_FAST_ARITH = 1u << 5,      /* tolerance mode (fp32, Muller kernels, SESPH) of the FORCE walk: reciprocals instead of
                                           IEEE divisions, v_rsq instead of correctly rounded square roots, float powers, fused
                                           multiply-adds (the density stays exact).  Hash / index / cell tables are unaffected
                                           (calcGridPos keeps its true division); densities, forces and the integrated state agree
                                           with the default reference-order IEEE arithmetic to ~1e-6 relative per step.  The
                                           reference itself is built with --use_fast_math (CMakeLists.txt:85).  Ignored (exact
                                           arithmetic) for fp64, Monaghan kernels, IISPH, PCISPH, PBF, DFSPH and NRS_FLAG_REFERENCE_ORDER. */
    NRS_FLAG_IISPH_SELF_BY_SLOT = 1u << 6, /* IISPH: computePressure / computePressureForce exclude the particle ITSELF from their
                                           neighbour sums.  The reference excludes the slot whose number equals the CUDA thread
                                           id instead (sph_kernel_impl.cuh:1412,1568), which makes its result depend
                                           on the ORDER of the input arrays: the same particles permuted differ by centimetres
                                           after four steps.  Default off = the reference's behaviour; a
                                           multi-GPU slab run can only be compared with a single-domain run with this flag on. */
    NRS_FLAG_NO_WALL_WORKGROUPS = 1u << 7, /* gather launches with ONE kind of workgroup: particles next to a wall are evaluated in place
                                           by the general (boundary-aware) code instead of by the wall workgroups that walk the step's
                                           wall list.  Same results bit for bit; slower on scenes with walls */
    NRS_FLAG_STAGED_SCAN = 1u << 8,     /* SESPH fp32 Muller: the density launch is the LDS-STAGED scan (k_density_staged: one wavefront
                                           per 64 consecutive sorted slots, row hulls by ballot + readlane, one z-plane of candidates
                                           staged in LDS) instead of the quantised global-memory scan.  Same lists, same sums, bit for
                                           bit; measured slower, kept as the north-star's literal kernel shape.
                                           Ignored by IISPH, PCISPH, PBF and DFSPH contexts (their one scan publishes the wide hit lists) */
    NRS_FLAG_IISPH_INPLACE_P = 1u << 1, /* reserved: the reference's racy in-place Jacobi is NOT
                                           offered; P_l is always double-buffered */
};

/* error codes */
enum {
    NRS_OK = 0,
    NRS_E_INVALID = -1,  /* bad argument */
    NRS_E_HIP = -2,      /* a HIP runtime call failed */
    NRS_E_CAPACITY = -3, /* more particles than nrs_config.capacity */
    NRS_E_STATE = -4,    /* call not valid in the context's current state */
    NRS_E_NODEVICE = -5, /* no usable HIP device */
    NRS_E_NOTREADY = -6, /* non-blocking query: the result is not there yet */
};

typedef struct nrs_config {
    uint32_t struct_size; /* = sizeof(nrs_config) */
    int32_t device;       /* HIP device ordinal; -1 = the calling thread's current device */
    int32_t solver;       /* NRS_SOLVER_* */
    int32_t precision;    /* 32 or 64: sizeof(SReal)*8 (DOUBLE_PRECISION) */
    int32_t kernel_set;   /* NRS_KERNELS_* (KERNEL_SET) */
    int32_t surface_tension; /* USE_SURFACE_TENSION (CMakeLists.txt:28) */
    uint32_t flags;       /* NRS_FLAG_* */
    uint32_t reserved;
    uint64_t capacity;    /* max fluid particles; run-time replacement of MAX_PARTICLE_NUMBER (sph/sph.h:19) */
    void *stream;         /* hipStream_t to launch on, or NULL to let the context create its own */
} nrs_config;

/* Pipeline stages, for nrs_step_partial / nrs_stage_ms.  Order is the order of SPH::update()
 * (sph/sph.cpp:233-284) and IISPH::update() (sph/iisph/iisph.cpp:172-216).  A PCISPH step is HASH, SORT, REORDER, DENSITY
 * (density only, no Tait pressure), then the P_* stages; nrs_step_partial on a PCISPH context accepts those and refuses the others.
 * PBF and DFSPH steps have the same stages (and the same refusals).  DFSPH: DENSITY also holds the factor launch (alpha), P_ADVECT
 * the divergence solve on the sorted velocities ahead of the advection launch, P_SOLVE the density solve on vel_adv, P_INTEGRATE
 * v = vel_adv, x += dt v. */
/* On a context whose boundary bodies move (nrs_set_boundary_bodies) NRS_STAGE_HASH also holds the step's rebuild of the boundary
 * tables on the device: pose + hash, radix sort, reorder, near-boundary bits. */
enum {
    NRS_STAGE_HASH = 1,      /* calcHash                     sph_cuda.cu:230 */
    NRS_STAGE_SORT = 2,      /* sortParticles                sph_cuda.cu:58 */
    NRS_STAGE_REORDER = 3,   /* reorderDataAndFindCellStart  sph_cuda.cu:295 */
    NRS_STAGE_DENSITY = 4,   /* computeDensityPressure kernel sph_kernel_impl.cuh:365 */
    NRS_STAGE_FORCES = 5,    /* computeForces kernel          sph_kernel_impl.cuh:609 */
    NRS_STAGE_INTEGRATE = 6, /* integrateSystem              sph_cuda.cu:211 */
    NRS_STAGE_P_ADVECT = 7,    /* PCISPH, PBF: non-pressure forces, vel_adv, first predicted positions, p (lambda) = 0 */
    NRS_STAGE_P_SOLVE = 8,     /* PCISPH: the predictive-corrective loop; PBF: the Jacobi projection (two launches per iteration) */
    NRS_STAGE_P_INTEGRATE = 9, /* PCISPH: v = vel_adv + dt Fp / m, x += dt v (iisph_integrate); PBF: v = (x* - x) / dt (+ XSPH), x = x* */
    NRS_STAGE_I_DENSITY = 10,      /* computeIisphDensity        sph_kernel_impl.cuh:770 */
    NRS_STAGE_I_DISPLACEMENT = 11, /* computeDisplacementFactor  :851 */
    NRS_STAGE_I_ADVECTION = 12,    /* computeAdvectionFactor     :1114 */
    NRS_STAGE_I_SOLVE = 13,        /* computeSumDijPj + computePressure loop, sph_cuda.cu:736-823 */
    NRS_STAGE_I_PFORCE = 14,       /* computePressureForce       :1497 */
    NRS_STAGE_I_INTEGRATE = 15,    /* iisph_integrate            :1625 */
    NRS_STAGE_COUNT = 16
};

/* Arrays readable through nrs_get_array / nrs_device_ptr.  "sorted" = in grid-hash order of the
 * current step, as the reference's m_dSorted* arrays (sph/sph.h:105-111). */
enum {
    NRS_ARR_POS = 0,        /* SVec4[N]  current particle positions (what the next update() starts from) */
    NRS_ARR_VEL = 1,        /* SVec4[N] */
    NRS_ARR_PRESSURE = 2,   /* SReal[N]  IISPH warm-start pressure (m_pressure, iisph.cpp:216) */
    NRS_ARR_HASH = 3,       /* uint32[N] sorted cell hashes (m_dGridParticleHash) */
    NRS_ARR_INDEX = 4,      /* uint32[N] sorted particle indices (m_dGridParticleIndex) */
    NRS_ARR_CELL_START = 5, /* uint32[numCells], 0xffffffff = empty */
    NRS_ARR_CELL_END = 6,   /* uint32[numCells], defined only where CELL_START != 0xffffffff */
    NRS_ARR_SORTED_POS = 7, /* SVec4[N] */
    NRS_ARR_SORTED_VEL = 8, /* SVec4[N] */
    NRS_ARR_DENS = 9,       /* SReal[N] */
    NRS_ARR_PRES = 10,      /* SReal[N] */
    NRS_ARR_FORCES = 11,    /* SVec4[N] (w=0) */
    NRS_ARR_B_HASH = 12,    /* boundary: uint32[Nb] */
    NRS_ARR_B_INDEX = 13,
    NRS_ARR_B_CELL_START = 14,
    NRS_ARR_B_CELL_END = 15,
    NRS_ARR_B_SORTED = 16,  /* SVec4[Nb]: xyz = sorted boundary position, w = its Vbi */
    NRS_ARR_DENS_ADV = 20,  /* IISPH (sph/iisph/iisph.h:27-41) */
    NRS_ARR_DENS_CORR = 21,
    NRS_ARR_P_L = 22,
    NRS_ARR_AII = 23,
    NRS_ARR_VEL_ADV = 24,
    NRS_ARR_FORCES_ADV = 25,
    NRS_ARR_FORCES_P = 26,
    NRS_ARR_DII_FLUID = 27,
    NRS_ARR_DII_BOUNDARY = 28,
    NRS_ARR_SUM_DIJ = 29,
    NRS_ARR_POS_PRED = 30,  /* PCISPH: SVec4[N] predicted positions x* of the last iteration.  On a PCISPH context NRS_ARR_VEL_ADV,
                               _FORCES_ADV, _FORCES_P (the pressure force), _DENS_CORR (the predicted density) and _P_L (the pressure p)
                               hold the PCISPH quantities; NRS_ARR_PRES and nrs_download(pres) the step's final pressures.
                               On a PBF context the same arrays hold the PBF quantities: _POS_PRED x*, _VEL_ADV, _FORCES_ADV,
                               _DENS_CORR rho*, _P_L lambda and _FORCES_P the correction dx of the last iteration; NRS_ARR_PRES
                               and nrs_download(pres) give lambda */
    NRS_ARR_VORTICITY = 31, /* PBF: SVec4[N] sorted (omega, |omega|) of the last step that had vorticity confinement on
                               (nrs_pbf_set_vorticity); NRS_E_STATE before there is one */
    NRS_ARR_DFSPH_ALPHA = 32,   /* DFSPH: SReal[N] sorted alpha = 1 / D of the last factor launch (NRS_E_STATE on other contexts
                                   and before a step).  On a DFSPH context NRS_ARR_DENS holds rho, _SORTED_VEL after P_ADVECT the
                                   divergence-free v, _VEL_ADV v* after the density solve, _FORCES_ADV the non-pressure forces,
                                   _DENS_CORR rho_adv and _P_L kappa of the last density iteration; NRS_ARR_PRES, NRS_ARR_PRESSURE and
                                   nrs_download(pres) hold K (m^2, the warm-start total; after a partial step up to P_ADVECT NRS_ARR_PRES
                                   is the sorted K_prev of the step).  NRS_ARR_POS_PRED is refused. */
    NRS_ARR_DFSPH_KAPPA_V = 33, /* DFSPH: SReal[N] sorted Kv, the divergence solve's total (after a partial step up to DENSITY the
                                   sorted Kv_prev of the step); NRS_E_STATE on other contexts and before a step */
    NRS_ARR_NORMALS = 34,   /* PCISPH, PBF, DFSPH: SVec4[N] sorted, xyz = the Akinci normal n_i and w = rho_i, of the last step that had
                               gamma > 0 (nrs_set_surface_akinci); NRS_E_STATE before there is one, and on SESPH and IISPH contexts */
    NRS_ARR_B_BODY = 35,    /* uint32[Nb]: the body id of every SORTED boundary particle (nrs_set_boundary_bodies); NRS_E_STATE without
                               an assignment.  On a context with bodies NRS_ARR_B_SORTED, _B_HASH, _B_INDEX and the boundary cell
                               tables show the pose of the last step */
};

const char *nrs_last_error(void);
/* library/ABI version: (major<<16)|minor */
uint32_t nrs_version(void);
/* number of HIP devices visible (0 if none / runtime unusable) */
int nrs_device_count(void);

/* Replaces SPH::SPH()/_initialize() device allocation (sph/sph.cpp:132-188, iisph.cpp:123-159).
 * `params` points to nrs_params_f32 or nrs_params_f64 according to cfg->precision. */
int nrs_create(const nrs_config *cfg, const void *params, nrs_ctx **out);
int nrs_destroy(nrs_ctx *ctx);

/* setParameters (sph/sph.cuh:40, sph_cuda.cu:183-187).  Changing gridSize/numCells re-allocates the
 * cell tables as SPH::_initializeGrid does (sph.cpp:193-202). */
int nrs_set_params(nrs_ctx *ctx, const void *params);
int nrs_get_params(nrs_ctx *ctx, void *params);

/* H2D of particle state: replaces the cudaMemcpy H2D at the top of update() (sph.cpp:233-234,
 * iisph.cpp:172-174).  Writes particles [first, first+count) and sets N = max(N, first+count).
 * vel4/pres may be NULL (zeros).  nrs_set_num_particles truncates/extends N within capacity. */
int nrs_upload_particles(nrs_ctx *ctx, const void *pos4, const void *vel4, const void *pres, uint64_t first,
                         uint64_t count);
int nrs_set_num_particles(nrs_ctx *ctx, uint64_t n);
uint64_t nrs_num_particles(nrs_ctx *ctx);

/* SPH::updateGpuBoundaries (sph/sph.cpp:391-432): upload boundary particles bi4 (SVec4[nb]) and volumes
 * vbi (SReal[nb]); if update_grid != 0 apply SPH::updateGrid (sph.cpp:313-337: origin = AABBmin-0.1,
 * gridSize = nextPow2(ceil((extent+0.1)/h))) and re-allocate the cell tables; then hash, sort and
 * build the boundary cell ranges.  nb = 0 clears the boundaries.  The (possibly new) grid is visible
 * through nrs_get_params. */
int nrs_set_boundaries(nrs_ctx *ctx, const void *bi4, const void *vbi, uint64_t nb, int update_grid);

/* ---- kinematic boundary bodies (DESIGN.md "Kinematic boundary bodies"; came after nrs_version() 0.3 without a version change) ----
 * The boundary particles of the last nrs_set_boundaries are grouped into rigid bodies whose poses the context advances at the start
 * of every step, x += dt v, q = exp(dt omega / 2) q with dt the step's time step, and whose boundary tables it rebuilds on the
 * device, on its stream, with no host wait.  The fluid sees the walls at the step's pose; DFSPH also sees their velocity.  One-way:
 * the fluid does not push back.
 * nrs_set_boundary_bodies: body_of[i] is the body of boundary particle i, in upload order.  Body 0 is the static world and is never
 * transformed; bodies 1 .. nbodies-1 are rigid.  The uploaded positions are each body's rest pose, its origin c_k the mean of its
 * rest positions.  body_of == NULL or nbodies <= 1 clears the assignment (the walls return to the uploaded positions), and so does
 * every later nrs_set_boundaries.  NRS_E_STATE before any nrs_set_boundaries and while a host-driven IISPH step is in progress;
 * NRS_E_INVALID for nb different from the context's boundary count, an id >= nbodies, nbodies > NRS_MAX_BODIES or a slab context
 * (nrs_slab_configure on a context with bodies fails the same way).
 * The grid is not re-derived: nrs_set_boundaries(update_grid) sees the rest poses only, the caller sizes it for the whole motion (a
 * body that leaves it wraps through the hash, as fluid particles do).  The volumes V_b are kept: they are invariant within a rigid
 * body; bodies that come to overlap each other are the caller's business.  The host classes' checkpoints do not hold poses. */
enum { NRS_MAX_BODIES = 16 };
int nrs_set_boundary_bodies(nrs_ctx *ctx, const uint32_t *body_of, uint64_t nb, uint32_t nbodies);
/* World-frame linear velocity of the body's origin and angular velocity about it, held until changed (default 0).  NRS_E_INVALID for
 * body 0, an unknown body, a NaN or an infinite value.  Does not wait for the device. */
int nrs_set_body_velocity(nrs_ctx *ctx, uint32_t body, const double v[3], const double omega[3]);
/* A teleport: origin x and orientation q = (w, x, y, z), normalised by the library (NRS_E_INVALID for a zero or non-finite one).  The
 * next step rebuilds the tables at this pose (after advancing it, if the body has a velocity). */
int nrs_set_body_pose(nrs_ctx *ctx, uint32_t body, const double x[3], const double q[4]);
/* The pose the last completed or enqueued step used (or the one set since). */
int nrs_get_body_pose(nrs_ctx *ctx, uint32_t body, double x[3], double q[4]);

/* update() x nsteps with state resident on the device (no per-step PCIe traffic).  Asynchronous for the caller: a call with
 * nsteps >= 2 hands the steps to a thread owned by the context and returns at once (before the device has finished, usually before
 * it has started); nsteps <= 1 enqueues the step on the calling thread and returns without waiting for the device.  Every other
 * nrs_* call on the context first waits until the queued steps have been enqueued, and nrs_synchronize / nrs_download /
 * nrs_get_array additionally wait for the device.  A call the context's state does not allow (mid-update after nrs_step_partial, a
 * host-driven IISPH step in progress) is refused at once with NRS_E_STATE; an error that a QUEUED step runs into is returned by the
 * next call on the context, and the steps queued behind it are dropped.
 * (Why a thread: the step loop reads one number back per step — the mover count that sizes the coherent re-sort's library calls, or
 * the IISPH solver's exit test, sph_cuda.cu:736-741 — so whoever enqueues it runs about one step ahead of the device, not nsteps
 * ahead.  NRS_FLAG_FULL_SORT SESPH contexts have no such read-back.) */
int nrs_step(nrs_ctx *ctx, int nsteps);
/* Test hook: run ONE update() but stop after `stop_stage` (NRS_STAGE_*), leaving the intermediate
 * arrays readable through nrs_get_array.  After a partial step the particle state is mid-update:
 * re-upload before stepping again. */
int nrs_step_partial(nrs_ctx *ctx, int stop_stage);
int nrs_synchronize(nrs_ctx *ctx);

/* D2H: replaces the cudaMemcpy D2H at the end of update() (sph.cpp:283-284, iisph.cpp:214-216).
 * Any pointer may be NULL.  Order = grid-hash order of the last step, as in the reference. */
int nrs_download(nrs_ctx *ctx, void *pos4, void *vel4, void *pres);
/* Viewer hand-off that does not stall the simulation (consumer: the render loop's getHostPos(), main.cpp:587-588;
 * the reference copies pos+vel back synchronously at the end of every update(), sph.cpp:283-284).
 * nrs_snapshot_begin copies the current positions (and velocities if with_vel != 0) device-to-device into a staging
 * buffer on the context's stream, then to page-locked host memory owned by the library on a separate copy stream:
 * steps enqueued afterwards overlap with the PCIe transfer.  Two snapshots can be in flight (a third call first waits
 * for the oldest).  nrs_snapshot_wait hands out the OLDEST pending snapshot: with block == 0 it returns
 * NRS_E_NOTREADY (not an error, nrs_last_error is not set) while the transfer is running.  The pointers stay valid
 * until two further nrs_snapshot_begin calls; *step = number of nrs_step steps the state had seen.  vel4 is NULL for
 * a snapshot taken without velocities. */
int nrs_snapshot_begin(nrs_ctx *ctx, int with_vel);
int nrs_snapshot_wait(nrs_ctx *ctx, int block, const void **pos4, const void **vel4, uint64_t *n, uint64_t *step);

/* Copy one of NRS_ARR_* to host memory (dst_bytes must be >= the array's size; returns it in *out_bytes
 * when dst == NULL). */
int nrs_get_array(nrs_ctx *ctx, int which, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
/* Device address of one of NRS_ARR_* (valid until the next call that re-allocates or swaps buffers,
 * i.e. read it after each step).  For zero-copy consumers (renderer VBO upload, halo packing). */
int nrs_device_ptr(nrs_ctx *ctx, int which, void **dptr, uint64_t *bytes);

/* IISPH / PCISPH / PBF / DFSPH: solver iterations of the last step (the `l` of sph_cuda.cu:736; DFSPH: the density solve's). */
int nrs_last_iterations(nrs_ctx *ctx, uint32_t *iters);
/* Cap on IISPH / PCISPH / PBF / DFSPH solver iterations per step.  0 = none for IISPH, as the reference; 0 = 50 for PCISPH and PBF
 * (their loops need not end; a PBF step in fixed-count mode ignores the cap); 0 = 100 for each of DFSPH's two loops (a loop in
 * fixed-count mode ignores it). */
int nrs_set_max_iterations(nrs_ctx *ctx, uint32_t max_iters);

/* PCISPH solver settings (NRS_E_STATE on any other context).  The loop stops after the iteration l with l >= min_iters and
 * max_i max(rho*_i - rho0, 0) / rho0 <= max_density_error, or at the iteration cap (nrs_set_max_iterations).  delta = 0: the
 * pressure scale delta is derived from a prototype particle on a cubic lattice of spacing prototype_spacing (0 = cbrt(m / rho0)),
 * evaluated on the device once per parameter change; delta > 0 is used as given.  Defaults: 0.01, 3, 0, 0.
 * NRS_E_INVALID for max_density_error <= 0, min_iters == 0 or a negative spacing / delta. */
int nrs_pcisph_configure(nrs_ctx *ctx, double max_density_error, uint32_t min_iters, double prototype_spacing, double delta);

/* PBF solver settings (NRS_E_STATE on any other context).  max_density_error > 0: the loop stops after the iteration l with
 * l >= min_iters and max_i max(rho*_i - rho0, 0) / rho0 <= max_density_error, or at the iteration cap (nrs_set_max_iterations,
 * 0 = 50).  max_density_error = 0: exactly min_iters iterations and nothing read back during the step (fixed-count mode).
 * relaxation: the constraint-force mixing term is eps = relaxation * D_proto, D_proto the constraint's gradient norm for a prototype
 * particle on the cubic lattice of spacing cbrt(m / rho0), evaluated on the device once per parameter change.  xsph: the XSPH
 * velocity smoothing factor c (0 = off).  Defaults: 0.01, 2, 0.01, 0.  NRS_E_INVALID for max_density_error < 0, min_iters == 0,
 * relaxation <= 0 or xsph outside [0, 1]. */
int nrs_pbf_configure(nrs_ctx *ctx, double max_density_error, uint32_t min_iters, double relaxation, double xsph);
/* PBF tensile correction (Macklin & Mueller's s_corr; NRS_E_STATE on any other context): on fluid pairs the position correction
 * uses lambda_i + lambda_j + s_ij, s_ij = -k (W(x*_i - x*_j) / W_q)^4 with W_q = W((dq h, 0, 0)).  Defaults k = 0 (off), dq = 0.2.
 * NRS_E_INVALID for a NaN or infinite value, k < 0, dq outside (0, 1) or a W_q that is not positive.  Came after nrs_version() 0.3
 * without a version change, as PBF did. */
int nrs_pbf_set_tensile(nrs_ctx *ctx, double k, double dq);
/* PBF vorticity confinement (NRS_E_STATE on any other context): at the end of the step vel_i += dt eps_v (N_i x omega_i),
 * DESIGN.md "PBF".  Default 0 (off).  NRS_E_INVALID for a NaN, infinite or negative eps_v. */
int nrs_pbf_set_vorticity(nrs_ctx *ctx, double eps_v);
/* DFSPH solver settings (NRS_E_STATE on any other context), DESIGN.md "DFSPH".  Each loop (the density solve, and the divergence
 * solve) stops after the iteration l with l >= its minimum and avg_i e_i <= its error, or at the iteration cap
 * (nrs_set_max_iterations, 0 = 100); an error of 0 runs exactly the minimum and reads nothing back during the step (fixed-count
 * mode).  e_i = max(rho_adv_i - rho0, 0) / rho0 in the density solve, max(dt div_i, 0) in the divergence solve.
 * min_divergence_iters = 0 turns the divergence solve off.  warm_start = 1: each solve starts with one extra pair of launches from
 * half the previous step's total (K, Kv).  Defaults: 1e-3, 2, 1e-3, 1, 1.  NRS_E_INVALID for a NaN, infinite or negative error,
 * min_iters == 0 or warm_start outside {0, 1}.  Came after nrs_version() 0.3 without a version change. */
int nrs_dfsph_configure(nrs_ctx *ctx, double max_density_error, uint32_t min_iters, double max_divergence_error,
                        uint32_t min_divergence_iters, int warm_start);
/* Implicit viscosity on a DFSPH context (NRS_E_STATE on any other), DESIGN.md "Implicit viscosity" (Weiler et al. 2018): behind the
 * advection launch the step solves (I - dt nu L) u = v* for the velocity and replaces vel_adv by u; the density solve, the integration
 * and everything after them are unchanged.  With x the step's start positions, DFSPH's neighbour rule and gradients g, rho of the
 * step's scan and x_ij = x_i - x_j,
 *   (A u)_i = u_i - dt nu          (rho0 / rho_i) 10 sum_j (rho0 / rho_j) ((u_i - u_j) . x_ij) / (|x_ij|^2 + 0.01 h^2) g_ij
 *                 - dt nu_boundary (rho0 / rho_i) 10 sum_b                ( u_i        . x_ib) / (|x_ib|^2 + 0.01 h^2) g_ib.
 * nu is the kinematic viscosity in m^2/s; nu_boundary the wall friction against walls at rest (0 = slip).  The solve is plain
 * conjugate gradients from u0 = v*, every sum in a fixed order.  It stops after the iteration l >= min_iters with
 * |r|^2 <= tolerance^2 |v*|^2, or at max_iters (0 = 100); |r|^2 is not read back before min_iters, and tolerance = 0 runs exactly
 * min_iters iterations and reads nothing back during the step.  nu = 0 (the default) switches the solve off and frees its buffers: the
 * step, its launches and its bits are then those of a context that never called this.  The explicit viscous term of the advection
 * launch keeps obeying params.viscosity: for the implicit term alone set params.viscosity to 0.
 * NRS_E_INVALID for a NaN, infinite or negative nu or nu_boundary, a tolerance outside [0, 1), tolerance = 0 with min_iters = 0, or
 * max_iters not 0 and below min_iters.  nu_boundary > 0 on a context whose boundary particles are grouped into moving bodies, and
 * nrs_set_boundary_bodies on a context with nu_boundary > 0, are NRS_E_STATE.  Came after nrs_version() 0.3 without a version change. */
int nrs_dfsph_set_viscosity(nrs_ctx *ctx, double nu, double nu_boundary, double tolerance, uint32_t min_iters, uint32_t max_iters);
/* What the last step's solve left: on (also filled when the call fails), the iterations that began with a nonzero residual,
 * residual = |r| of the last iteration and rhs_norm = |v*|, read from the device on request (the call waits for the stream).  Any
 * pointer may be NULL.  NRS_E_STATE before a step with the solve on. */
int nrs_dfsph_viscosity_info(nrs_ctx *ctx, int *on, uint32_t *iterations, double *residual, double *rhs_norm);

/* Surface tension and wall adhesion of Akinci, Akinci and Teschner (2013) on a PCISPH, PBF or DFSPH context (NRS_E_STATE on SESPH and
 * IISPH contexts, whose steps are the reference's), DESIGN.md "Akinci surface tension and adhesion": the advection stage's force_adv
 * gains -gamma m sum_j K_ij (m C(r_ij) r_ij / |r_ij| + n_i - n_j) - beta_adhesion m sum_b psi_b A(r_ib) r_ib / |r_ib|, with the normals
 * n_i = h sum_j (m / rho_j) grad W(r_ij), K_ij = 2 rho0 / (rho_i + rho_j) and the kernels Cakinci / Aboundary of the parameter block's
 * ksurf1, ksurf2, bpol.  While gamma > 0 the reference-style cohesion term of nrs_config.surface_tension is left out (two cohesion
 * models do not stack).  Defaults 0, 0 (off: the step, its launches and its bits are those of a context that never called this).
 * NRS_E_INVALID for a NaN, infinite or negative value.  Came after nrs_version() 0.3 without a version change, as PBF did. */
int nrs_set_surface_akinci(nrs_ctx *ctx, double gamma, double beta_adhesion);

/* Per-stage device time, measured with HIP events recorded on the context's stream around the stage's
 * launches.  stage_mask: bit s set = time NRS_STAGE_s (0 = off, 0xffffffff = every stage).  nrs_set_profiling also
 * resets the accumulated times.  nrs_stage_ms returns the time of that stage summed over all steps since the last
 * nrs_set_profiling call and how many launches of the stage that covers; it synchronizes the stream (nrs_step itself
 * does not: event pairs are resolved lazily).  `launches` counts the event brackets of the stage, not kernels: a stage's launches of a
 * step share one bracket (a continuation later in the step adds time, not a count); a context that tracks its particles (nrs_track_*)
 * records its gather in a bracket of its own in NRS_STAGE_REORDER, whose count is then one higher per step and whose time is the sum. */
int nrs_set_profiling(nrs_ctx *ctx, uint32_t stage_mask);
int nrs_stage_ms(nrs_ctx *ctx, int stage, float *ms, uint32_t *launches);

/* ---- multi-GPU slab decomposition (new; the reference is single-GPU — SURVEY §8e) ---------------------------
 * One context per rank/GPU.  A rank owns the particles whose GLOBAL grid cell-x index (floor((x-origin.x)/cell.x),
 * same SphSimParams on every rank) lies in [cell_lo, cell_hi).  Per step, before nrs_step:
 *   nrs_slab_pack   partitions the current particles (stable, deterministic): owned ones are compacted, leavers and
 *                   the halo_cells-wide border layers are written to the two caller-owned DEVICE message buffers;
 *   (caller)        exchanges the buffers with the left/right neighbour — RCCL send/recv over xGMI, e.g.
 *                   torch.distributed.batch_isend_irecv on the tensors that own the buffers;
 *   nrs_slab_unpack appends the received migrants (they become owned) and halo copies (read-only, pos.w = 2).
 * nrs_step then evaluates density on owned particles plus one cell beyond each cut and forces on owned particles
 * only.  Message buffer: nrs_slab_message_bytes(capacity, precision) bytes =
 *   [u32 nMigrants, u32 nHalo, u32 0, u32 0 | vec4 pos[capacity] | vec4 vel[capacity]].
 * Pass NULL for the neighbour that does not exist (ends of the chain).  IISPH contexts: halo_cells >= 8 and the step is driven
 * through nrs_iisph_predict / _iterate / _finish (below). */
int nrs_slab_configure(nrs_ctx *ctx, int32_t cell_lo, int32_t cell_hi, int32_t halo_cells); /* NRS_E_INVALID on a PCISPH, PBF or DFSPH context */
/* counts (optional) receives {stay, migrate-left, halo-left, migrate-right, halo-right, ghost}.
 * With counts == NULL nrs_slab_pack does not wait for the device: the two messages are complete in stream order when it returns (the
 * caller enqueues its sends on the same stream right behind it), and the stream populations are read back together with the headers of
 * the received messages inside nrs_slab_unpack — ONE host synchronisation per exchange.  A message-capacity overflow is then reported
 * by nrs_slab_unpack (or by whichever call on the context comes first) with NRS_E_CAPACITY.  nrs_slab_last_counts returns the counts
 * of the last pack afterwards.  Passing counts makes nrs_slab_pack wait for them itself. */
int nrs_slab_pack(nrs_ctx *ctx, void *send_left, void *send_right, uint64_t capacity, uint32_t counts[6]);
int nrs_slab_unpack(nrs_ctx *ctx, const void *recv_left, const void *recv_right, uint64_t capacity);
int nrs_slab_last_counts(nrs_ctx *ctx, uint32_t counts[6]);
/* owned particles (the first nrs_num_owned() entries of NRS_ARR_POS/VEL right after nrs_slab_pack/unpack) */
uint64_t nrs_num_owned(nrs_ctx *ctx);
uint64_t nrs_slab_message_bytes(uint64_t capacity, int precision);
/* Owned particles (pos.w == 1) per global cell-x column first_cell .. first_cell+ncells-1, to host memory: the input
 * of a count-balanced re-cut.  New cuts are applied by calling nrs_slab_configure again; particles that now belong
 * to a neighbour leave with the next nrs_slab_pack (a cut may therefore move by less than a slab width at a time). */
int nrs_slab_histogram(nrs_ctx *ctx, int32_t first_cell, uint32_t ncells, uint32_t *counts);

/* IISPH step in three calls, for runs in which the solver loop's exit test needs a value the library cannot form alone — a slab
 * run: pressureSolve (sph_cuda.cu:736-741) loops `while ((rho_avg - 1000) > 1 || l < 2)` with rho_avg the average predicted
 * density over ALL particles, i.e. over all ranks.
 *   nrs_iisph_predict   hash / sort / reorder + predictAdvection (density, displacement factors, advection factors)
 *   nrs_iisph_iterate   ONE relaxed-Jacobi iteration; returns the sum of the corrected densities over the particles this rank
 *                       owns and their number (all particles of a single-domain context): the caller adds these up over the
 *                       ranks (one scalar all-reduce), forms rho_avg = (SReal)sum / count and decides
 *   nrs_iisph_finish    pressure force + integration
 * nrs_step on an IISPH context is the same three phases with the loop inside.  Slab runs (nrs_slab_configure on an IISPH context)
 * need a halo of at least 2 * iterations + 4 cells — every iteration consumes two cells of halo validity, the predict stages three,
 * the pressure force one — i.e. >= 8; nrs_iisph_iterate fails with NRS_E_STATE when the loop runs longer than the halo supports.
 * The warm-start pressure of every particle travels in vel.w of the slab messages (iisph_integrate zeroes vel.w anyway). */
int nrs_iisph_predict(nrs_ctx *ctx); /* (the three: NRS_E_STATE on any other context) */
int nrs_iisph_iterate(nrs_ctx *ctx, double *sum_density_corr, uint64_t *count);
int nrs_iisph_finish(nrs_ctx *ctx);

/* Coherent re-sort statistics since nrs_create: steps whose (hash, index) pairs were produced by sorting only the
 * particles that changed cell and merging them into the rest, and how many of those fell back to the full radix sort
 * because more than half of the particles had moved (the measured break-even).  (Steps after an upload
 * or a grid change and partial steps always use the full sort and are not counted.) */
int nrs_resort_stats(nrs_ctx *ctx, uint64_t *steps, uint64_t *fallbacks);

/* Diagnostics of the last completed step, as doubles (they synchronize the stream):
 *   NRS_STAT_MOVERS         particles that changed grid cell (the mover count of the last coherent re-sort; -1 if the
 *                           last step sorted from scratch without counting)
 *   NRS_STAT_HIT_OVERFLOW   particles whose neighbour hit list overflowed (they take the reference-order cell walk)
 *   NRS_STAT_HIT_MEAN/_MAX  neighbours (fluid + boundary hits) per particle kept in the hit lists
 *   NRS_STAT_UNSTAGED       particles whose wavefront could not stage its neighbour rows in LDS (grid-edge cells, or
 *                           hulls longer than the pool) and scanned them from global memory instead
 *   NRS_STAT_DENSITY_ERROR  PCISPH, PBF: max_i max(rho*_i - rho0, 0) / rho0 after the last iteration of the last step (a PBF step
 *                           in fixed-count mode forms it when it is asked for)
 *   NRS_STAT_PCISPH_DELTA   PCISPH: the pressure scale delta the last step used
 *   NRS_STAT_PBF_EPSILON    PBF: the constraint-force mixing term eps the last step used
 *   NRS_STAT_DENSITY_ERROR  on DFSPH: max_i e_i of the last density iteration
 *   NRS_STAT_DFSPH_DENSITY_AVG           DFSPH: avg_i e_i of the last density iteration
 *   NRS_STAT_DFSPH_DIVERGENCE_AVG        DFSPH: avg_i e_i of the last divergence iteration (NRS_E_STATE when the solve is off)
 *   NRS_STAT_DFSPH_DIVERGENCE_ITERATIONS DFSPH: divergence iterations of the last step (nrs_last_iterations gives the density solve's)
 *   NRS_STAT_SLAB_PARTITION kind of the last nrs_slab_pack: 0 = compacting (the owned particles were moved to the front), 1 = in
 *                           place (they kept their slots), 2 = in place from the classification the last step's force kernel left;
 *                           NRS_E_STATE before the first pack.  Read-only, does not touch the device.  Came after nrs_version() 0.3
 *                           without a version change.
 * The DFSPH values are formed on request from the e_i the solve left.
 * The HIT_* / UNSTAGED values need the shared hit lists of the production kernels (NRS_E_STATE otherwise); the PCISPH / PBF / DFSPH
 * values a context of that kind that has completed a solve. */
enum { NRS_STAT_MOVERS = 0, NRS_STAT_HIT_OVERFLOW = 1, NRS_STAT_HIT_MEAN = 2, NRS_STAT_HIT_MAX = 3, NRS_STAT_UNSTAGED = 4,
       NRS_STAT_DENSITY_ERROR = 5, NRS_STAT_PCISPH_DELTA = 6, NRS_STAT_PBF_EPSILON = 7, NRS_STAT_DFSPH_DENSITY_AVG = 8,
       NRS_STAT_DFSPH_DIVERGENCE_AVG = 9, NRS_STAT_DFSPH_DIVERGENCE_ITERATIONS = 10, NRS_STAT_SLAB_PARTITION = 11 };
int nrs_get_stat(nrs_ctx *ctx, int which, double *out);

/* ---- field sampling (DESIGN.md "Field sampling"; came after nrs_version() 0.3 without a version change) -------------------------------
 * Evaluates the SPH fields of the CURRENT particle state (what nrs_download would return now) at positions that are not particles: at
 * caller-supplied points, or on the nodes of a regular lattice.  Read-only: a context that samples steps bit-identically to one that
 * never did.  Every solver, both precisions, both kernel sets; not on a slab context (NRS_E_INVALID: its arrays hold halo copies).
 *
 * With h = interactionRadius, m = particleMass and the neighbours j of a position x those fluid particles with length(x - x_j) < h
 * (difference in SReal, the float length() of the kernels):
 *   NRS_FIELD_DENSITY   SReal[M]      rho(x) = sum_j m W(x - x_j), W the density kernel of the context's kernel set; with
 *                                     NRS_FIELD_WALLS also sum_b (restDensity V_b) W(x - x_b) over the boundary particles within h, at
 *                                     the walls' current pose
 *   NRS_FIELD_GRADIENT  SVec4[M]      grad rho(x) = sum_j m grad W(x - x_j), fluid only, w = 0; a neighbour AT x contributes nothing
 *   NRS_FIELD_VELOCITY  SVec4[M]      Shepard average (sum_j (m W_j) v_j) / (sum_j m W_j), w = the fluid-only denominator; all four
 *                                     components 0 where the denominator is 0
 *   NRS_FIELD_COUNT     uint32_t[M]   number of fluid neighbours
 *   NRS_FIELD_WALLS     modifier of NRS_FIELD_DENSITY only; ignored on a context without boundary particles
 * One accumulator per output component; the cells of the position's 3x3x3 neighbourhood are visited z, y, x ascending, the sorted
 * particles of a cell ascending, a cell's boundary particles after its fluid particles: results are deterministic and do not depend
 * on the entry point.  A position with a non-finite coordinate gets zeros and count 0.
 *
 * nrs_sample_points: m positions (HOST SVec4[m], w ignored).  nrs_sample_lattice: node (i, j, k) of the lattice is at
 * (SReal)(origin[a] + idx[a] * spacing[a]) (formed in double, rounded once) and has the linear index (k * dims[1] + j) * dims[0] + i.
 * Both enqueue on the context's stream and do not wait for the device (nrs_sample_points returns once its points are copied).
 * nrs_sample_result copies a field of the LAST sample call to the host and waits, as nrs_get_array does (dst NULL: only the size);
 * nrs_sample_device_ptr gives its device address, as nrs_device_ptr does.  Both stay valid until the next sample call,
 * nrs_sample_release (frees every sampler buffer; the next sample call allocates again) or nrs_destroy.  The sampler keeps its own
 * sorted copy of the particles and its own cell table; they are rebuilt only when the particles, the grid or the boundaries changed
 * since the last sample call; nrs_sample_builds gives the number of builds since nrs_create (read-only, does not touch the device).
 *
 * NRS_E_STATE: mid-update after nrs_step_partial; a host-driven IISPH step in progress; a result or pointer of a field the last
 * sample call did not compute (or before any).  NRS_E_INVALID: fields without an output flag or with unknown bits; points4 NULL with
 * m > 0; m >= 2^31; a spacing that is not finite or <= 0, an origin that is not finite, a dim of 0 or more than 2^31 nodes; a slab
 * context; a grid whose cellSize is below h in some axis (the 27-cell walk is then incomplete), whose gridSize is below 4 in some axis
 * or is not a power of two (the hash's wrap then aliases cells of one row and a neighbour would be counted twice).  m == 0 succeeds
 * with empty results; a context without particles gives zeros. */
enum { NRS_FIELD_DENSITY = 1, NRS_FIELD_GRADIENT = 2, NRS_FIELD_VELOCITY = 4, NRS_FIELD_COUNT = 8, NRS_FIELD_WALLS = 16 };
typedef struct nrs_lattice { double origin[3]; double spacing[3]; uint32_t dims[3]; uint32_t reserved; } nrs_lattice;
int nrs_sample_points(nrs_ctx *ctx, const void *points4, uint64_t m, uint32_t fields);
int nrs_sample_lattice(nrs_ctx *ctx, const nrs_lattice *lattice, uint32_t fields);
int nrs_sample_result(nrs_ctx *ctx, uint32_t field, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
int nrs_sample_device_ptr(nrs_ctx *ctx, uint32_t field, void **dptr, uint64_t *bytes);
int nrs_sample_release(nrs_ctx *ctx);
int nrs_sample_builds(nrs_ctx *ctx, uint64_t *builds);

/* ---- surface extraction (DESIGN.md "Surface extraction"; came after nrs_version() 0.3 without a version change) ------------------------
 * The iso-surface rho = iso of the sampled density as an indexed triangle mesh, by marching tetrahedra on the nodes of a lattice, all
 * on the device.  nrs_surface_extract IS nrs_sample_lattice(ctx, lattice, DENSITY [| GRADIENT] [| VELOCITY] [| WALLS]) followed by the
 * mesher: it writes the sampler's own result arrays (nrs_sample_result(ctx, NRS_FIELD_DENSITY, ...) afterwards returns exactly the
 * lattice the mesh was cut from), every refusal and the cache rule of the sampler apply, nrs_sample_builds counts as for any sample
 * call.  Read-only like the sampler.  Every output is bit-reproducible: nothing below depends on a launch geometry.
 *
 * Nodes.  Lattice, node positions and linear node index are nrs_sample_lattice's.  A node is INSIDE when rho(node) >= (SReal)iso.
 * Cells.  The cube with low corner (i, j, k), i < dims[0] - 1, j < dims[1] - 1, k < dims[2] - 1, cells ordered by the linear index of
 *   their low corner.  Each is split into the six Kuhn tetrahedra: for a permutation (a, b, c) of the axes the corners 000, +e_a,
 *   +e_a+e_b, 111 (tet-local numbers 0..3), permutations in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx.  All six share the body
 *   diagonal and neighbouring cells agree on every face diagonal, so there are no ambiguous cases.
 * Vertices.  Every node owns the seven lattice edges towards +, numbered (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1),
 *   those whose far node exists.  An owned edge whose ends differ in inside-ness carries one vertex; vertices are numbered by owner
 *   node ascending, then edge number ascending.  With p0, f0 position and density of the owner and p1, f1 of the far node, in SReal:
 *   t = (iso - f0) / (f1 - f0), x = p0 + t * (p1 - p0) per component (the library is built without contraction: two roundings).  The
 *   record is SVec4 (x, y, z, t).
 * Triangles.  Three uint32_t vertex numbers; listed by cell ascending, then tet, then within the tet.  A tet with one corner inside,
 *   or three, gives one triangle over its three crossing edges.  One with inside corners a < b and outside corners c < d gives the quad
 *   ac, ad, bd, bc split along ac-bd into (ac, ad, bd) and (ac, bd, bc).  Every triangle is wound so that its right-hand normal points
 *   from the inside corners to the outside ones (out of the fluid).  A surface that does not reach the lattice boundary is a closed,
 *   consistently oriented manifold; one cut by the boundary is open there.
 * Attributes (flags).  NRS_SURFACE_GRADIENT / NRS_SURFACE_VELOCITY: the sampler's gradient / velocity record at the two end nodes,
 *   interpolated as g0 + t * (g1 - g0) on all four components, one SVec4 per vertex.  Not normalised: the outward normal is -g / |g|.
 *   NRS_SURFACE_WALLS: the density includes the wall term (NRS_FIELD_WALLS).
 *
 * nrs_surface_extract needs the totals to size its outputs: it WAITS for the context's stream once (queued nrs_step work included) and
 * reads back eight bytes.  *vertices / *triangles (either may be NULL) get V and T.  An empty surface is a success with V = T = 0 and
 * zero-byte results.  nrs_surface_result copies ONE result (an NRS_MESH_* id) to the host and waits (dst NULL: only the size):
 * SVec4[V] vertices / gradient / velocity, uint32_t[3 T] triangles; nrs_surface_device_ptr gives its device address (NULL for zero
 * bytes).  The mesh buffers belong to the mesher: valid until the next extract, nrs_surface_release (frees only the mesher's buffers)
 * or nrs_destroy; nrs_sample_* calls and nrs_sample_release do not touch them.  Nothing is allocated before the first extract.
 *
 * NRS_E_INVALID: iso not finite or <= 0; unknown flag bits; a lattice dim below 2; more than 2^27 nodes (7 vertices and 12 triangles
 * per node then fit 32-bit offsets); a `which` that is not exactly one result id; everything nrs_sample_lattice refuses as invalid.
 * NRS_E_STATE: a result or pointer before any extract or after nrs_surface_release, or of an attribute the last extract did not
 * compute; mid-update after nrs_step_partial; a host-driven IISPH step in progress. */
enum { NRS_SURFACE_GRADIENT = 1, NRS_SURFACE_VELOCITY = 2, NRS_SURFACE_WALLS = 4 };
enum { NRS_MESH_VERTICES = 1, NRS_MESH_TRIANGLES = 2, NRS_MESH_GRADIENT = 4, NRS_MESH_VELOCITY = 8 };
int nrs_surface_extract(nrs_ctx *ctx, const nrs_lattice *lattice, double iso, uint32_t flags, uint64_t *vertices, uint64_t *triangles);
int nrs_surface_result(nrs_ctx *ctx, uint32_t which, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
int nrs_surface_device_ptr(nrs_ctx *ctx, uint32_t which, void **dptr, uint64_t *bytes);
int nrs_surface_release(nrs_ctx *ctx);

/* ---- diffuse particles (DESIGN.md "Diffuse particles"; came after nrs_version() 0.3 without a version change) --------------------------
 * Spray, foam and air bubbles after Ihmsen, Akinci, Akinci, Teschner (2012), "Unified spray, foam and air bubbles for particle-based
 * fluids": a set of secondary particles that the context owns and nrs_diffuse_step advances, all on the device.  It never runs inside
 * nrs_step.  It READS the current fluid state (what nrs_download would return now) through the field sampler's particle grid (the
 * sampler's cache rule applies and nrs_sample_builds counts a rebuild; the sampler's result arrays are not touched) and writes only its
 * own buffers: a context that uses it steps bit-identically to one that never did.  Every output is bit-reproducible: offsets come from
 * scans, nothing depends on a launch geometry or on the order of atomics.  DESIGN.md states every formula and the order of every sum.
 *
 * One nrs_diffuse_step(ctx, dt) (dt == 0: the context's timestep), per fluid particle i in the sampler's SORTED order (cell hash
 * ascending, ties by array index), every sum over the fluid neighbours j != i with length(x_i - x_j) < h, W_lin = 1 - |x_ij| / h:
 *   normals     g_i = sum_j m grad W(x_i - x_j): the sampler's gradient at the particle (NRS_DIFFUSE_NORMALS holds g_i, the density
 *               gradient, w = 0).  The unit normal the potentials use points OUT of the fluid: n_i = -g_i / |g_i|.
 *   trapped air sum |v_ij| (1 - vhat_ij . xhat_ij) W_lin
 *   wave crest  sum (1 - n_i . n_j) W_lin over the j with xhat_ji . n_i < 0, the whole sum gated by vhat_i . n_i >= 0.6
 *   energy      1/2 m |v_i|^2
 *   A zero-length vector has no direction: that term, or that gate, is 0.  Each potential x is clamped to
 *   I = (min(x, tau_max) - min(x, tau_min)) / (tau_max - tau_min); rate = I_k (k_ta I_ta + k_wc I_wc) particles per second;
 *   births_i = min(floor(rate dt + u), max_per_particle), u the particle's first uniform draw.
 * Then the living diffuse particles are advected: the sampler's Shepard velocity vt and neighbour count n at the particle decide —
 * n < spray_below: spray, ballistic under gravity; n > bubble_above: bubble, v += dt (-k_buoyancy g) + k_drag (vt - v); else foam,
 * carried with vt and losing dt of its lifetime.  A particle dies when its lifetime is <= 0 or a coordinate is not finite or leaves
 * the grid box [worldOrigin, worldOrigin + gridSize * cellSize).  Survivors are compacted in their order (oldest first); the births
 * follow, ordered by fluid slot, then birth number, each on a random point of the cylinder of radius particleRadius and height
 * dt |v_i| along v_i, with velocity v_i + the radial offset (NOT divided by dt) and a lifetime uniform in lifetime[].  Births that do
 * not fit the capacity are the LAST in that order; they are counted in `dropped`.  New particles are not advected in their birth step;
 * their kind is that of their parent's neighbour count (the parent included).  Uniforms: a counter-based integer hash of (seed,
 * diffuse steps since configure, fluid slot, draw number), top 24 bits times 2^-24.  There are no collisions with boundary particles.
 *
 * nrs_diffuse_configure checks and stores the configuration and allocates nothing; it restarts the step counter and `dropped`, and
 * keeps the living particles when the capacity is unchanged (drops them otherwise).  nrs_diffuse_step enqueues on the context's stream
 * and does not wait; buffers are allocated by the first step or upload.  nrs_diffuse_count WAITS and gives the living count, the count
 * per kind (0 spray, 1 foam, 2 bubble) and the births refused for capacity since configure (any pointer may be NULL).
 * nrs_diffuse_result copies ONE result to the host and waits (dst NULL: only the size); nrs_diffuse_device_ptr gives its device address
 * (NULL for zero bytes); both wait for the living count.  D: living diffuse particles; N: fluid particles of the last diffuse step:
 *   NRS_DIFFUSE_POS        SVec4[D], w = remaining lifetime         NRS_DIFFUSE_POTENTIALS  SVec4[N] (I_ta, I_wc, I_k, births per second)
 *   NRS_DIFFUSE_VEL        SVec4[D], w = 0                          NRS_DIFFUSE_BIRTHS      uint32_t[N]
 *   NRS_DIFFUSE_KIND       uint32_t[D], as found by the last step   NRS_DIFFUSE_NORMALS     SVec4[N]
 * (the three per-fluid arrays are in the sampler's sorted order; they are kept for tests and tuning).  nrs_diffuse_upload replaces the
 * living set with n <= capacity particles (pos4.w = lifetime; listed as spray until a step classifies them) and waits.
 * nrs_diffuse_release frees the buffers and empties the set; the configuration stays.
 *
 * NRS_E_INVALID: a NULL or wrongly sized config, capacity 0 or above 2^30, a tau range that is not finite with min < max, negative or
 * non-finite k_ta / k_wc, lifetime not 0 <= min <= max, k_drag outside [0, 1], max_per_particle outside [1, 1024], reserved != 0; a
 * NaN or negative dt; N * max_per_particle above 2^31; an upload above the capacity; a slab context and the sampler's grid conditions;
 * an unknown result id.  NRS_E_STATE: anything before nrs_diffuse_configure; a per-fluid result before the first step; mid-update
 * after nrs_step_partial; a host-driven IISPH step in progress.  What is wrong with an argument is named before the state. */
typedef struct nrs_diffuse_config {
    uint32_t struct_size, capacity;          /* max diffuse particles; 0 is invalid */
    uint64_t seed;
    double tau_ta[2], tau_wc[2], tau_k[2];   /* clamp ranges of the three potentials, min < max */
    double k_ta, k_wc;                       /* particles per second at potential 1 */
    double lifetime[2];                      /* foam lifetime drawn uniformly in [min, max] seconds */
    double k_buoyancy, k_drag;               /* bubbles; k_drag in [0, 1] */
    uint32_t spray_below, bubble_above;      /* kinds by fluid-neighbour count n: n < spray_below spray, n > bubble_above bubble, else foam */
    uint32_t max_per_particle, reserved;     /* cap on births per fluid particle per step, >= 1 */
} nrs_diffuse_config;
enum { NRS_DIFFUSE_POS = 0, NRS_DIFFUSE_VEL = 1, NRS_DIFFUSE_KIND = 2, NRS_DIFFUSE_POTENTIALS = 3, NRS_DIFFUSE_BIRTHS = 4, NRS_DIFFUSE_NORMALS = 5 };
int nrs_diffuse_configure(nrs_ctx *ctx, const nrs_diffuse_config *cfg);
int nrs_diffuse_step(nrs_ctx *ctx, double dt);
int nrs_diffuse_count(nrs_ctx *ctx, uint64_t *alive, uint64_t by_kind[3], uint64_t *dropped);
int nrs_diffuse_result(nrs_ctx *ctx, uint32_t which, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
int nrs_diffuse_device_ptr(nrs_ctx *ctx, uint32_t which, void **dptr, uint64_t *bytes);
int nrs_diffuse_upload(nrs_ctx *ctx, const void *pos4, const void *vel4, uint64_t n);
int nrs_diffuse_release(nrs_ctx *ctx);

/* ---- sources and sinks (DESIGN.md "Sources and sinks"; came after nrs_version() 0.3 without a version change) ---------------------------
 * Emitters append fluid particles on the device, kill volumes remove them; both change the particle count without a host round trip.
 * The feature is opt-in: a context that never configures it allocates nothing new and launches nothing new.
 *
 * WHEN.  At the top of every step of nrs_step and of nrs_iisph_predict — before the bodies move, before the step's kernels are chosen,
 * and, when an enabled emitter exists, also on an empty context (it steps from empty) — first the sinks cull, then the emitters emit.
 * dt is the context's timestep.  A step in which the context is still empty afterwards does nothing else.
 *
 * EMITTERS.  Up to NRS_MAX_EMITTERS slots.  d = direction / |direction| (double).  Frame: e1 = normalised d x axis, axis the coordinate
 * axis of d's smallest absolute component (the lowest on a tie), e2 = d x e1 (all double, in the order written).  s = spacing, or, for
 * spacing 0, cbrt(particleMass / restDensity) of the parameters at nrs_emitter_set.  Sites of a layer: integer (i, j), j-major (j outer,
 * i inner, both ascending); rect: |i| <= floor(half_extent[0] / s), |j| <= floor(half_extent[1] / s); disc: both within
 * floor(r / s), r = half_extent[0], keeping (i s)^2 + (j s)^2 <= r^2.  Schedule per slot and step, on the host in double:
 *   acc += speed * dt;  while (acc >= s) { acc -= s; emit a layer with origin o = center + acc * d; }
 * The layers of a step are appended in that order, slots ascending.  A layer that does not fit capacity - n whole, or that would take
 * the slot past max_particles, is not emitted: its sites are added to `dropped`, the accumulator still advances (no burst later).
 * A site's position component a is (SReal)(o[a] + (i * s) * e1[a] + (j * s) * e2[a]), evaluated in double in the written order without
 * contraction and rounded once (the lattice-node rule of nrs_sample_lattice; the same bits in all four builds); pos.w = 1;
 * vel = (SReal)(speed * d[a]), w = 0; pressure 0; DFSPH Kv 0.  Emitting into occupied space is the caller's business.
 * nrs_emitter_set(slot, NULL) removes a slot; every successful set restarts the slot's accumulator and counts.  nrs_emitter_get returns
 * the emitter as stored (direction normalised, spacing as given) and its counts; any pointer may be NULL; an empty slot reads as zeros.
 * nrs_emit_block appends the nodes of a lattice in its linear index order ((k * dims[1] + j) * dims[0] + i), positions by the lattice
 * rule, all with velocity (SReal)vel[a]: all of them or, with NRS_E_CAPACITY, none.
 *
 * SINKS.  A particle is removed when a coordinate of its position is not finite; or, with NRS_SINK_DOMAIN, when a coordinate lies
 * outside [worldOrigin, worldOrigin + gridSize * cellSize); or when it lies inside a box (min <= x < max on every axis).  The
 * comparisons are in SReal against bounds rounded to SReal once (the domain's upper bound is formed in double from the parameters).
 * Survivors keep their order; positions, velocities, pressures and DFSPH's Kv move together.  The cull before a step runs before step
 * k = interval, 2 interval, ... counted from nrs_sinks_set (interval 0 = 1).  It reads the survivor count back: one wait on the stepping
 * thread.  If nothing was removed nothing else happens: the step is bit-identical to that of a context without sinks.  nrs_cull runs
 * one cull now with the current sinks (non-finite positions are removed even with none) and waits.  nrs_sinks_count: particles removed
 * and culls run since nrs_sinks_set.
 *
 * After any emission or removal the arrays are in the state nrs_upload_particles leaves: the next step hashes and sorts in full, and
 * the field sampler, the mesher and the diffuse particles rebuild their grid.
 *
 * NRS_E_INVALID: a slab context (and nrs_slab_configure on a context with sources or sinks); a slot >= NRS_MAX_EMITTERS; an unknown
 * shape; a non-finite field; a zero direction; speed < 0; spacing < 0, or so small that a layer has more than 2^24 sites; a negative
 * extent; nboxes > NRS_MAX_SINK_BOXES; unknown flags; reserved != 0; a box with min >= max on some axis; a bad lattice or a non-finite
 * velocity for nrs_emit_block.  NRS_E_STATE: mid-update after nrs_step_partial; a host-driven IISPH step in progress (nrs_cull,
 * nrs_emit_block).  NRS_E_CAPACITY: nrs_emit_block with more nodes than capacity - n.  A refused call changes nothing. */
enum { NRS_MAX_EMITTERS = 16, NRS_MAX_SINK_BOXES = 16 };
enum { NRS_EMITTER_RECT = 0, NRS_EMITTER_DISC = 1 };
typedef struct nrs_emitter {
    uint32_t shape, enabled;
    double center[3], direction[3];   /* direction normalised by the library */
    double half_extent[2];            /* rect: along e1, e2; disc: [0] = radius */
    double speed, spacing;            /* spacing 0 = cbrt(particleMass / restDensity) */
    uint64_t max_particles;           /* 0 = no limit */
} nrs_emitter;
int nrs_emitter_set(nrs_ctx *ctx, uint32_t slot, const nrs_emitter *e);
int nrs_emitter_get(nrs_ctx *ctx, uint32_t slot, nrs_emitter *e, uint64_t *emitted, uint64_t *dropped);
int nrs_emit_block(nrs_ctx *ctx, const nrs_lattice *sites, const double vel[3], uint64_t *added);

enum { NRS_SINK_DOMAIN = 1 };
typedef struct nrs_sink_config {
    uint32_t flags, nboxes, interval, reserved;   /* interval 0 = 1: cull before every interval-th step */
    double boxes[NRS_MAX_SINK_BOXES][6];          /* min xyz, max xyz; inside means min <= x < max */
} nrs_sink_config;
int nrs_sinks_set(nrs_ctx *ctx, const nrs_sink_config *cfg);   /* NULL clears */
int nrs_cull(nrs_ctx *ctx, uint64_t *removed);
int nrs_sinks_count(nrs_ctx *ctx, uint64_t *removed_total, uint64_t *culls);

/* Akinci boundary volumes on the device (no context needed): vbi[i] = 1 / sum_k W_poly6(|x_i - x_k|, h) over the boundary
 * particles k within h of i, i included — what the reference takes from its un-vendored submodule
 * (sample_spheres::boundary_forces::getVbi, main.cpp:546; own implementation, parity unpinned).  bi4: nb xyzw particles of
 * SReal (precision 32/64), vbi: nb SReal, both HOST buffers; device < 0 = current device.  Uses the same hash / radix sort /
 * cell-range / 27-cell gather as the solver, on a private grid. */
int nrs_boundary_volumes(int device, int precision, const void *bi4, uint64_t nb, double h, void *vbi);

/* Test hook: the DEVICE smoothing kernels / vector helpers (common/kernels_impl.cuh:85-203, helper_math.h semantics) on n
 * caller-supplied separations r3 (and second vectors s3, may be NULL), HOST buffers of 3n SReal; which = 0 Wdefault, 1
 * Wdefault_grad, 2 Wpressure_grad, 3 Wviscosity_grad, 4 Wmonaghan, 5 Wmonaghan_grad, 6 Cakinci (c0 = ksurf1, c1 = ksurf2), 7 Aboundary
 * (c0 = bpol; the reference's unclamped form: NaN where roundoff leaves its radicand negative), 8 dot, 9 length, 10 vec*float,
 * 11 float*vec, 12 vec/float, 13 identity, 14 +, 15 - (the numbering of oracle/ref_kernels_driver.cpp; scalars land in out[3i]).  Lets the
 * tests compare the product's arithmetic bit for bit with the reference's own header compiled unmodified. */
int nrs_eval_smoothing(int precision, int which, uint64_t n, const void *r3, const void *s3, double h, double c0, double c1, void *out);

/* maxDensity / maxVelocity (sph/sph.cuh, sph_cuda.cu:32-53): diagnostics over the sorted arrays. */
int nrs_max_density(nrs_ctx *ctx, double *out);
int nrs_max_velocity(nrs_ctx *ctx, double *out_speed);

/* ---- anisotropic surface reconstruction (DESIGN.md "Anisotropic kernels"; Yu & Turk 2013; came without a version change) ------------------
 * The raw SPH density of an under-dense scene dips below any usable iso value between the particles: its iso-surface is a foam of small
 * closed surfaces.  Here the field the mesher is fed is a volume-normalised colour field (about 1 inside the fluid whatever the
 * density) of kernels whose centres are smoothed towards the neighbourhood's weighted mean and which are stretched along the principal
 * axes of the neighbourhood's covariance.  Geometry only: nothing depends on the kernel set, the particle mass or the rest density.
 * Read-only for the simulation; it uses the sampler's particle grid (its cache rule, nrs_sample_builds) and the mesher unchanged.
 * R is the build's real type, h = interactionRadius; r = (R)2 h, the largest centre shift is h / 2, the largest semi-axis 3 h / 2.
 *
 * Pass A, one record per fluid particle i in the sampler's sorted order.  Candidates: the fluid particles j of the 5 x 5 x 5 unwrapped
 * cell neighbourhood of x_i (i included), cells z, y, x ascending, sorted slots ascending, one accumulator per component.  d = x_j - x_i
 * per component in R, d2 = (dx dx + dy dy) + dz dz; j is a neighbour when d2 < r2 = r r; count = the neighbours.  w = 1 - (|d| / r)^3;
 * Sw = sum w, M = sum w d, S = sum w d d^T, D = sum (r2 - d2)^3.  V_i = 1 / (k6 D), k6 = 315 / (64 pi r^9).  mu = M / Sw,
 * delta = lambda mu, scaled to length h / 2 if longer; centre = x_i + delta.  C = S / Sw - mu mu^T = U diag(s1 >= s2 >= s3) U^T.  With
 * count < n_eps or s1 not > 0 the semi-axes are a_k = k_n support; otherwise st_k = max(s_k, s1 / k_r) and
 * a_k = support st_k / cbrt(st_1 st_2 st_3); then a_k = min(a_k, 3 h / 2).  G = U diag(1 / a_k) U^T, weight = (315 / (64 pi)) V_i /
 * (a1 a2 a3), bound = max a_k.  A particle with a non-finite coordinate has count 0, weight 0, bound 0, G = 0.
 *   NRS_ANISO_CENTER  SVec4[N]     centre, bound
 *   NRS_ANISO_G       SVec4[2N]    (G00, G01, G02, G11), (G12, G22, weight, 0)
 *   NRS_ANISO_COUNT   uint32_t[N]  neighbour count
 *   NRS_ANISO_INDEX   uint32_t[N]  the particle's index in nrs_download order
 * Pass B, the field at a lattice node x (the sampler's node rule): the same walk around x; d = x - centre_j, skipped unless
 * d2 < bound_j^2; g = G_j d, q2 = g . g, skipped unless q2 < 1; p = 1 - q2.  phi = sum weight_j p^3; grad phi = sum -6 weight_j p^2 (G_j g);
 * velocity = (sum (weight_j p^3) v_j) / phi with w = phi, all four components 0 where phi is 0.  A non-finite node gets zeros.
 *
 * nrs_aniso_config: NULL means support = h, lambda = 0.9, k_r = 4, k_n = 0.5, n_eps = 25; a support of 0 means h.
 * nrs_aniso_build runs pass A (enqueues only; the records are recomputed on every call).  nrs_aniso_result copies ONE result to the
 * host and waits (dst NULL: only the size); nrs_aniso_device_ptr gives its device address; the buffers are valid until the next build,
 * nrs_aniso_release (frees only these buffers) or nrs_destroy.  nrs_surface_extract_aniso runs pass A, then pass B on the lattice INTO
 * THE SAMPLER'S RESULT ARRAYS (NRS_FIELD_DENSITY holds phi; GRADIENT / VELOCITY with NRS_SURFACE_GRADIENT / _VELOCITY;
 * nrs_sample_result afterwards returns exactly the lattice the mesh was cut from), then the mesher of nrs_surface_extract: the mesh
 * comes back through nrs_surface_result / nrs_surface_device_ptr.  iso is a value of phi (0.5 is the usual choice).
 *
 * Refusals: everything nrs_sample_lattice and nrs_surface_extract refuse; NRS_E_INVALID for NRS_SURFACE_WALLS, a gridSize < 8 on some
 * axis (the five cells of a row would alias through the wrap), support outside (0, 1.5 h], lambda outside [0, 1], k_r < 1, k_n outside
 * (0, 1], a non-finite field, reserved != 0.  NRS_E_STATE: a result or pointer before any build or after nrs_aniso_release. */
enum { NRS_ANISO_CENTER = 1, NRS_ANISO_G = 2, NRS_ANISO_COUNT = 4, NRS_ANISO_INDEX = 8 };
typedef struct nrs_aniso_config { double support, lambda, k_r, k_n; uint32_t n_eps, reserved; } nrs_aniso_config;
int nrs_aniso_build(nrs_ctx *ctx, const nrs_aniso_config *cfg);
int nrs_aniso_result(nrs_ctx *ctx, uint32_t which, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
int nrs_aniso_device_ptr(nrs_ctx *ctx, uint32_t which, void **dptr, uint64_t *bytes);
int nrs_aniso_release(nrs_ctx *ctx);
int nrs_surface_extract_aniso(nrs_ctx *ctx, const nrs_lattice *lattice, double iso, uint32_t flags, const nrs_aniso_config *cfg,
                              uint64_t *vertices, uint64_t *triangles);

/* ---- particle identity and attributes (DESIGN.md "Particle identity and attributes"; came without a version change) ------------------------
 * Every step returns its arrays in that step's grid-hash order, emitters append and kill volumes remove: nothing else tells the caller
 * which particle is which afterwards.  With tracking enabled the context keeps, per fluid particle and in the order of NRS_ARR_POS /
 * nrs_download (the "current order"):
 *   id      uint32_t, unique within the context's life (until the next nrs_track_enable); NRS_TRACK_NONE is never an id
 *   birth   uint32_t, the number of completed steps at the moment the particle entered, saturating at 0xffffffff
 *   record  one SVec4 of user data, only with NRS_TRACK_ATTR
 * Opt-in: nothing is allocated before nrs_track_enable, and a context that never enables it launches what it always launched.  A
 * tracked context steps bit-identically to an untracked one.  Every solver, both precisions, both kernel sets; not on a slab context.
 *
 * HOW THE STATE MOVES.  A step: one launch behind the reorder gathers new[s] = old[index[s]] (index: NRS_ARR_INDEX of that step) for
 * id, birth and the record; the buffers swap at the end of the step, so a partial step (nrs_step_partial) leaves the tracked arrays of
 * the last completed state in place.  Emission: the particle of a launch's site t gets id = first + t (emitters: layer-major, layers
 * in schedule order, slots ascending; nrs_emit_block: the lattice's linear index), birth = completed steps, record = the slot's emit
 * value.  Cull: survivors keep id, birth, record and their order.  nrs_upload_particles(first, count): slots below the old n keep
 * id, birth and record (the same particle, moved); slots at or above the old n get fresh consecutive ids in slot order, birth =
 * completed steps and the emit value of slot -1.  nrs_set_num_particles: shrinking drops the tail, growing makes the new slots fresh
 * the same way.  Ids are never reused.  A call or step that would pass id 0xfffffffe fails with NRS_E_CAPACITY and changes nothing
 * (nrs_track_enable renumbers).
 *
 * nrs_track_enable numbers the n particles now present 0 .. n-1 in the current order, birth 0, record zeros, next_id = n, emit values
 * zeros; calling it again renumbers and resets (that is how flags are changed).  nrs_track_disable drains the stream and frees the
 * buffers.  nrs_track_info never refuses (any pointer may be NULL).
 * nrs_track_upload overwrites slots [first, first + count) of NRS_TRACK_ID, _BIRTH (uint32_t) or _ATTRIBUTE (SVec4) from host memory
 * and waits; for ids next_id becomes the larger of itself and one plus the largest uploaded id.  UNIQUENESS OF UPLOADED IDS IS THE
 * CALLER'S BUSINESS.  It is the call that carries identity across a context rebuild.
 * nrs_track_result copies one array to the host and waits (dst NULL: only the size); nrs_track_device_ptr gives its device address.
 * A consumer on the context's stream needs no wait; the pointers are valid until the next enable, disable or nrs_destroy, and have
 * to be asked for again after every step, cull and nrs_track_diffuse (the buffers swap).  NRS_TRACK_SLOT_OF names the result of the
 * last nrs_track_locate; its pointer is valid only until the next nrs_track_locate (a larger one reallocates).
 * nrs_track_emit_value: slots 0 .. NRS_MAX_EMITTERS-1 hold the record given to each emitter's particles, slot -1 serves
 * nrs_emit_block, appended uploads and count growth; the default is zeros (values are rounded to SReal).
 * nrs_track_locate(first_id, count) answers "where is id k now": uint32_t slot_of[count], NRS_TRACK_NONE where id first_id + k does
 * not live, else its slot in the current order; count <= 2^27, 0 gives an empty result.  Enqueues and returns.
 *
 * nrs_track_diffuse: one explicit Euler step of da/dt = kappa_c lap a on channel c of the record (dye mixing, heat conduction).
 * Never part of nrs_step; it does not touch the simulation state.  dt == 0: the context's timestep.  A channel with kappa_c == 0 is
 * copied.  It runs on the field sampler's particle grid (its refusals and cache rule apply, nrs_sample_builds counts a rebuild).  With
 * h = interactionRadius, m = particleMass, rho0 = restDensity, R = SReal, rho the sampler's density at the particles (with
 * NRS_FIELD_WALLS when the context has boundary particles), eta2 = (R)0.01 * (h * h), per particle i over the fluid particles j != i of
 * its 27 cells (cells z, y, x ascending, sorted slots ascending, one accumulator per channel):
 *   d = x_i - x_j; len = length(d) (float); skipped unless len < h; skipped if len == 0
 *   g = grad W(d); dot = d.x g.x + d.y g.y + d.z g.z; r = (R)len; w = (m / (rho_i * rho_j)) * (dot / (r * r + eta2))
 *   acc_c += (a_i[c] - a_j[c]) * w
 *   a_new[c] = a_i[c] + ((((R)2 * (R)dt) * (R)kappa_c) * rho0) * acc_c
 * (the Laplacian of Brookshaw / Cleary and Monaghan with a uniform coefficient; w_ij == w_ji bit for bit, so a pair exchanges equal
 * and opposite amounts before the sums round).  A particle with a non-finite position keeps its record.  STABILITY IS NOT CHECKED:
 * the step obeys a maximum principle only while lambda_i = 2 dt kappa_c rho0 sum_j |w_ij| <= 1 for every particle.
 *
 * NRS_E_STATE: everything but nrs_track_enable, _disable and _info before nrs_track_enable; a record call (nrs_track_emit_value,
 * nrs_track_diffuse, NRS_TRACK_ATTRIBUTE) without NRS_TRACK_ATTR; a result, pointer, locate or diffuse mid-update after
 * nrs_step_partial or while a host-driven IISPH step is in progress (then also nrs_track_enable and nrs_track_upload);
 * NRS_TRACK_SLOT_OF before any locate.  NRS_E_INVALID: unknown flag bits; a slab context (and nrs_slab_configure on a tracking
 * context); an unknown `which`; an upload outside [0, n) or with a NULL source; an uploaded id of NRS_TRACK_NONE; a slot outside
 * -1 .. NRS_MAX_EMITTERS-1; count above 2^27; a negative or non-finite kappa or dt.  A refused call changes nothing. */
enum { NRS_TRACK_ATTR = 1u };                                   /* flags of nrs_track_enable */
enum { NRS_TRACK_ID = 0, NRS_TRACK_BIRTH = 1, NRS_TRACK_ATTRIBUTE = 2, NRS_TRACK_SLOT_OF = 3 };
#define NRS_TRACK_NONE 0xffffffffu
int nrs_track_enable(nrs_ctx *ctx, uint32_t flags);
int nrs_track_disable(nrs_ctx *ctx);
int nrs_track_info(nrs_ctx *ctx, int *on, uint32_t *flags, uint64_t *next_id);
int nrs_track_upload(nrs_ctx *ctx, uint32_t which, const void *src, uint64_t first, uint64_t count);
int nrs_track_result(nrs_ctx *ctx, uint32_t which, void *dst, uint64_t dst_bytes, uint64_t *out_bytes);
int nrs_track_device_ptr(nrs_ctx *ctx, uint32_t which, void **dptr, uint64_t *bytes);
int nrs_track_emit_value(nrs_ctx *ctx, int32_t slot, const double a[4]);
int nrs_track_locate(nrs_ctx *ctx, uint64_t first_id, uint64_t count);
int nrs_track_diffuse(nrs_ctx *ctx, const double kappa[4], double dt);

/* ---- mesh sampling (DESIGN.md "Mesh sampling"; came after nrs_version() 0.3 without a version change) ------------------------------------
 * The inverse of the surface extraction: a triangle mesh in, a signed-distance classification on a lattice and the selected lattice
 * nodes as particles out.  nrs_mesh_field and nrs_mesh_particles need no context (like nrs_boundary_volumes; device < 0 = the current
 * device); nrs_emit_mesh is nrs_emit_block restricted to the selected nodes.  Brute force: every node against every triangle, no
 * acceleration structure.  Deterministic: no atomics, every output is bit-reproducible.
 *
 * INPUT.  vertices: 3 nv doubles; triangles: 3 nt indices, wound counter-clockwise seen from outside; both HOST arrays.  Node
 * (i, j, k) of the lattice has the linear index (k * dims[1] + j) * dims[0] + i and the position P[a] = origin[a] + (double)i_a *
 * spacing[a] (the lattice rule of nrs_sample_lattice, kept in double).
 *
 * ARITHMETIC.  All of it is double, in the order written, without contraction; u.v = u.x v.x + u.y v.y + u.z v.z left to right;
 * u x v = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x).  Per node P the triangles t = 0 .. nt-1 ascending, (A, B, C) its
 * corners:
 *   WINDING (the generalised winding number, van Oosterom and Strackee's solid angle).  a = A - P, b = B - P, c = C - P;
 *     la = sqrt(a.a), lb = sqrt(b.b), lc = sqrt(c.c);  num = a . (b x c);
 *     den = la * lb * lc + (a.b) * lc + (b.c) * la + (c.a) * lb  (summed left to right);  acc += 2 * atan2(num, den), one accumulator;
 *     at the end w = acc / (4.0 * M_PI).  About 1 inside a closed mesh, about 0 outside, in between near holes.
 *   CLOSEST POINT (Ericson, Real-Time Collision Detection 5.1.5).  ab = B - A, ac = C - A, ap = P - A, bp = P - B, cp = P - C;
 *     d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp;
 *     vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4.  The first matching region wins:
 *       1. d1 <= 0 && d2 <= 0:                        q = A
 *       2. d3 >= 0 && d4 <= d3:                       q = B
 *       3. vc <= 0 && d1 >= 0 && d3 <= 0:             q = A + (d1 / (d1 - d3)) * ab
 *       4. d6 >= 0 && d5 <= d6:                       q = C
 *       5. vb <= 0 && d2 >= 0 && d6 <= 0:             q = A + (d2 / (d2 - d6)) * ac
 *       6. va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0:   q = B + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (C - B)
 *       7. otherwise dn = 1 / (va + vb + vc):         q = A + ab * (vb * dn) + ac * (vc * dn)   (left to right, per component)
 *     r = P - q, dd = r.r.  The candidate replaces the best only if dd < best (strict): ties keep the lower triangle index and a NaN
 *     (a triangle without area can produce one) never wins.  best starts at +inf with index 0xffffffff.
 * Only atan2 is not an IEEE-exact operation: dist2, nearest and closest3 are the same bits wherever these formulas are evaluated,
 * winding is bit-reproducible from run to run on one library.  A node's result does not depend on how the nodes are batched.
 *
 * nrs_mesh_field writes, for every node in linear index order, to the HOST arrays that are not NULL: winding (w), dist2 (best),
 * nearest (its triangle) and closest3 (its q, 3 doubles).  With winding NULL no atan2 is evaluated, with the other three NULL no
 * closest point.  All four NULL: the arguments are checked, nothing runs.
 *
 * SELECTION.  A node is selected iff its side is selected (NRS_MESH_INSIDE: w > 0.5; NRS_MESH_OUTSIDE: w <= 0.5; both: every node) and
 * dmin * dmin <= dist2 <= dmax * dmax (dmax may be +inf).  Fill with clearance: INSIDE, dmin = clearance, dmax = inf.  Wall shell:
 * INSIDE | OUTSIDE, 0, thickness.  NRS_MESH_SNAP emits the closest point q instead of the node: a smooth single layer on the surface
 * instead of a staircase.  SNAPPED POINTS MAY COINCIDE along sharp edges and at corners (several nodes share one closest point); Akinci
 * volumes (nrs_boundary_volumes) share the volume between coincident samples, so such a shell is a valid wall.  The selected nodes
 * keep the linear index order (a scan, no atomics).  A particle's component is (SReal)P[a], or (SReal)q[a] with SNAP, rounded once;
 * its w is 1.
 * nrs_mesh_particles: pos4 is a HOST array of `capacity` SVec4 of the given precision; *count is always set; pos4 NULL: count only;
 * count > capacity: nothing is written, NRS_E_CAPACITY.
 * nrs_emit_mesh appends the selected nodes behind the context's n exactly as nrs_emit_block appends all nodes (velocity (SReal)vel[a],
 * pressure 0, DFSPH Kv 0; tracking: consecutive ids in selection order, the emit value of slot -1): all of them or, with
 * NRS_E_CAPACITY (more than capacity - n selected), none.  The selection stays on the device; the call reads one number back, the
 * count, and frees its scratch buffers before it returns (it waits for the append).
 *
 * NRS_E_INVALID: a NULL mesh, vertices or triangles; nv == 0; nt == 0 or nt >= 2^31; an index >= nv; a non-finite vertex; a bad
 * lattice (as nrs_sample_lattice); a NULL rule, flags without a side or with unknown bits, reserved != 0, dmin < 0 or NaN, dmax NaN or
 * below dmin; a precision that is not 32 or 64; for nrs_emit_mesh also SNAP and everything nrs_emit_block refuses (NRS_E_STATE
 * likewise).  A refused call changes nothing. */
typedef struct nrs_mesh { const double *vertices; uint64_t nv; const uint32_t *triangles; uint64_t nt; } nrs_mesh;
/* flags of nrs_mesh_rule (macros: the NRS_MESH_* enumerators are the results of the surface extraction) */
#define NRS_MESH_INSIDE 1u
#define NRS_MESH_OUTSIDE 2u
#define NRS_MESH_SNAP 4u
typedef struct nrs_mesh_rule { uint32_t flags, reserved; double dmin, dmax; } nrs_mesh_rule;
int nrs_mesh_field(int device, const nrs_mesh *mesh, const nrs_lattice *lattice, double *winding, double *dist2, uint32_t *nearest,
                   double *closest3);
int nrs_mesh_particles(int device, int precision, const nrs_mesh *mesh, const nrs_lattice *lattice, const nrs_mesh_rule *rule, void *pos4,
                       uint64_t capacity, uint64_t *count);
int nrs_emit_mesh(nrs_ctx *ctx, const nrs_mesh *mesh, const nrs_lattice *lattice, const nrs_mesh_rule *rule, const double vel[3],
                  uint64_t *added);

#ifdef __cplusplus
}
#endif
#endif /* NEREUS_HIP_H */
