// nrs_ctx_base.h — what the C ABI translation unit (nrs_abi.hip) and the per-variant context translation units
// (nrs_inst_*.hip) share: HIPCHK on top of the error plumbing (nrs_error.h), the owners of device memory, pinned host memory and
// events, the abstract context.
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "nrs_error.h"

namespace nrs {

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(NRS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                       std::to_string(__LINE__) + ")");                                  \
    } while (0)

// The three owners below free what they hold when they go out of scope, on every path: nothing else in the library calls hipFree,
// hipHostFree or hipEventDestroy on them.  Move-only; a moved-from owner is empty.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int alloc(size_t n)
    {
        if (n <= bytes && p) return NRS_OK;
        release();
        if (n == 0) return NRS_OK;
        HIPCHK(hipMalloc(&p, n));
        bytes = n;
        return NRS_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value, "a DevBuf owns its allocation");

// page-locked host memory; reads like the T * it holds.  The user calls hipHostMalloc on .p, so a failure names the call that made it.
template <typename T> struct PinnedBuf {
    T *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~PinnedBuf() { release(); }
    void release() { if (p) (void)hipHostFree((void *)p); p = nullptr; }
    operator T *() const { return p; }
};

// a hipEvent_t the user creates in .e; reads like one
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { release(); }
    void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// hipSetDevice for the duration of a call that is not bound to a context's own device bookkeeping (nrs_boundary_volumes,
// nrs_eval_smoothing): the caller's current device is put back on every way out.  device < 0 = stay on the current device.
struct DeviceScope {
    int prev = -1;
    bool good = true;
    explicit DeviceScope(int device)
    {
        if (device < 0) return;
        good = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess;
        if (!good) prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    bool ok() const { return good; }
};

struct CtxBase {
    virtual ~CtxBase() {}
    virtual int init(const nrs_config &cfg, const void *params) = 0;
    virtual int set_params(const void *params) = 0;
    virtual int get_params(void *params) = 0;
    virtual int upload(const void *pos4, const void *vel4, const void *pres, uint64_t first, uint64_t count) = 0;
    virtual int set_n(uint64_t n) = 0;
    virtual uint64_t get_n() = 0;
    virtual int set_boundaries(const void *bi4, const void *vbi, uint64_t nb, int update_grid) = 0;
    virtual int set_boundary_bodies(const uint32_t *bodyOf, uint64_t nb, uint32_t nbodies) = 0;
    virtual int set_body_velocity(uint32_t body, const double *v, const double *omega) = 0;
    virtual int set_body_pose(uint32_t body, const double *x, const double *q) = 0;
    virtual int get_body_pose(uint32_t body, double *x, double *q) = 0;
    virtual int step(int nsteps, int stop) = 0;
    virtual int sync() = 0;
    virtual int download(void *pos4, void *vel4, void *pres) = 0;
    virtual int snapshot_begin(int withVel) = 0;
    virtual int snapshot_wait(int block, const void **pos4, const void **vel4, uint64_t *n, uint64_t *step) = 0;
    virtual int array(int which, void **dptr, uint64_t *bytes) = 0;
    virtual int stage_ms(int stage, float *ms, uint32_t *launches) = 0;
    virtual int reduce_max(int which, double *out) = 0;
    virtual int slab_configure(int lo, int hi, int halo) = 0;
    virtual int slab_pack(void *sendL, void *sendR, uint64_t cap, uint32_t *counts) = 0;
    virtual int slab_unpack(const void *recvL, const void *recvR, uint64_t cap) = 0;
    virtual uint64_t num_owned() = 0;
    virtual int slab_histogram(int lo0, uint32_t nbins, uint32_t *out) = 0;
    virtual void resort_stats(uint64_t *steps, uint64_t *fallbacks) = 0;
    virtual int get_stat(int which, double *out) = 0;
    virtual int iisph_phase(int phase, double *sum, uint64_t *count) = 0;
    virtual int pcisph_configure(double eta, uint32_t minIters, double spacing, double delta) = 0;
    virtual int pbf_configure(double eta, uint32_t minIters, double relaxation, double xsph) = 0;
    virtual int pbf_set_tensile(double k, double dq) = 0;
    virtual int pbf_set_vorticity(double epsV) = 0;
    virtual int dfsph_configure(double eta, uint32_t minIters, double etaV, uint32_t minItersV, int warm) = 0;
    virtual int set_surface_akinci(double gamma, double beta) = 0;
    virtual int dfsph_set_viscosity(double nu, double nuB, double tol, uint32_t minIters, uint32_t maxIters) = 0;
    virtual int dfsph_viscosity_info(int *on, uint32_t *iterations, double *residual, double *rhsNorm) = 0;
    virtual int settle() = 0;                           // finish host bookkeeping a previous call deferred (nrs_slab_pack's totals)
    virtual int slab_last_counts(uint32_t *counts) = 0; // stream populations of the last nrs_slab_pack
    virtual int set_profiling(uint32_t mask) = 0;
    // field sampling (nrs_kernels_sample.h; the host decisions: nrs_host_sample.h)
    virtual int sample_points(const void *points4, uint64_t m, uint32_t fields) = 0;
    virtual int sample_lattice(const nrs_lattice *lattice, uint32_t fields) = 0;
    virtual int sample_result(uint32_t field, void *dst, uint64_t dstBytes, uint64_t *outBytes) = 0;
    virtual int sample_device_ptr(uint32_t field, void **dptr, uint64_t *bytes) = 0;
    virtual int sample_release() = 0;
    virtual uint64_t sample_builds() = 0;
    // surface extraction (nrs_kernels_surface.h; the host decisions: nrs_host_surface.h)
    virtual int surface_extract(const nrs_lattice *lattice, double iso, uint32_t flags, uint64_t *vertices, uint64_t *triangles) = 0;
    virtual int surface_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) = 0;
    virtual int surface_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) = 0;
    virtual int surface_release() = 0;
    virtual int aniso_build(const nrs_aniso_config *cfg) = 0;
    virtual int aniso_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) = 0;
    virtual int aniso_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) = 0;
    virtual int aniso_release() = 0;
    virtual int surface_extract_aniso(const nrs_lattice *lattice, double iso, uint32_t flags, const nrs_aniso_config *cfg, uint64_t *vertices,
                                      uint64_t *triangles) = 0;
    // diffuse particles (nrs_kernels_diffuse.h; the host decisions: nrs_host_diffuse.h)
    virtual int diffuse_configure(const nrs_diffuse_config *cfg) = 0;
    virtual int diffuse_step(double dt) = 0;
    virtual int diffuse_count(uint64_t *alive, uint64_t *byKind, uint64_t *dropped) = 0;
    virtual int diffuse_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) = 0;
    virtual int diffuse_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) = 0;
    virtual int diffuse_upload(const void *pos4, const void *vel4, uint64_t n) = 0;
    virtual int diffuse_release() = 0;
    // sources and sinks (nrs_kernels_inflow.h; the host decisions: nrs_host_inflow.h)
    virtual int emitter_set(uint32_t slot, const nrs_emitter *e) = 0;
    virtual int emitter_get(uint32_t slot, nrs_emitter *e, uint64_t *emitted, uint64_t *dropped) = 0;
    virtual int emit_block(const nrs_lattice *lattice, const double *vel, uint64_t *added) = 0;
    virtual int emit_mesh(const nrs_mesh *mesh, const nrs_lattice *lattice, const nrs_mesh_rule *rule, const double *vel, uint64_t *added) = 0;
    virtual int sinks_set(const nrs_sink_config *cfg) = 0;
    virtual int cull(uint64_t *removed) = 0;
    virtual int sinks_count(uint64_t *removedTotal, uint64_t *culls) = 0;
    // particle identity and attributes (nrs_kernels_track.h; the host decisions: nrs_host_track.h)
    virtual int track_enable(uint32_t flags) = 0;
    virtual int track_disable() = 0;
    virtual int track_info(int *on, uint32_t *flags, uint64_t *nextId) = 0;
    virtual int track_upload(uint32_t which, const void *src, uint64_t first, uint64_t count) = 0;
    virtual int track_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) = 0;
    virtual int track_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) = 0;
    virtual int track_emit_value(int32_t slot, const double *a) = 0;
    virtual int track_locate(uint64_t firstId, uint64_t count) = 0;
    virtual int track_diffuse(const double *kappa, double dt) = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int device = 0;
    uint32_t lastIters = 0, maxIters = 0;
    uint32_t profMask = 0;
};

// one context class per (precision, kernel set), each compiled in its own translation unit (nrs_inst_*.hip)
template <typename R, int KSET> CtxBase *make_ctx2(bool surf);

} // namespace nrs
