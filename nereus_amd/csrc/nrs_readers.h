// nrs_readers.h — the owner of the three add-ons that only READ the particle state (include/nereus_hip.h; DESIGN.md "Field sampling",
// "Surface extraction", "Diffuse particles"): it holds the FieldSampler (nrs_field_sampler.h), the SurfaceMesher (nrs_surface_mesher.h)
// and the DiffuseSystem (nrs_diffuse.h) and has the entry points of nrs_sample_*, nrs_surface_* and nrs_diffuse_*.  It depends on the
// precision and the kernel set; the context (nrs_ctx_impl.h) holds one, checks its own state (validate) and tells it, per call, what the
// fluid is now (FluidNow).  Nothing a step owns is written.  Here once: the sampler's particle grid, rebuilt when its cache rule says so,
// as a GridView (grid); the one path of a sample call, nrs_surface_extract's too (sample_queries); the copy of a result to the host
// (copy_out).  The refusals, sizes and routes are nrs_host_sample.h's, nrs_host_surface.h's and nrs_host_diffuse.h's.
#pragma once
#include <climits>
#include <cstring>

#include "nrs_aniso.h"
#include "nrs_diffuse.h"
#include "nrs_field_sampler.h"
#include "nrs_surface_mesher.h"

namespace nrs {

// the fluid as the context sees it at the time of a call
template <typename R> struct FluidNow {
    typedef typename Vec4T<R>::type T4;
    const Params<R> &P;              // the kernels' parameters
    const T4 *pos, *vel; uint64_t n; // the current arrays and their living particles
    SampleKey key;                   // what the sampler's grid depends on (the cache rule)
    SampleFacts facts;               // what a refusal depends on
    const uint32_t *bCellStart, *bCellEnd; // the boundary's cell table
    const T4 *bSorted; uint64_t bCount;    // ... and its sorted particles
    hipStream_t stream;
};

template <typename R, int KSET> struct FluidReaders {
    typedef typename Vec4T<R>::type T4;
    static constexpr int PRECISION = (int)(8 * sizeof(R));
    FieldSampler sm;
    SurfaceMesher sf;
    DiffuseSystem df;
    AnisoSurface an;

    // ---- shared -----------------------------------------------------------------------------------------------------------------------
    // The sampler's grid of f's particles, rebuilt if the cache rule asks for it, as the kernels see it; walls: with the boundary's tables
    int grid(const FluidNow<R> &f, bool walls, GridView<R> &G)
    {
        if (sm.cache.needs_build(f.key)) {
            NRSCHK(sm.template build_grid<R>(f.P, f.pos, f.vel, f.n, f.stream));
            sm.cache.built(f.key);
        }
        std::memset(&G, 0, sizeof(G));
        G.cellStart = sm.cell_start(); G.cellEnd = sm.cell_end();
        G.nSorted = sm.sorted_count();
        G.err = sm.err_word();
        G.actLo = INT_MIN; G.actHi = INT_MAX;
        if (walls) { G.bCellStart = f.bCellStart; G.bCellEnd = f.bCellEnd; G.sB = f.bSorted; }
        return NRS_OK;
    }
    // `sz` bytes at the device pointer p to dst, waited for.  dst null: the size alone.  errWord, unless null: the run guard of the walks
    // that wrote p, read along; set: it is cleared and the call fails with errText
    static int copy_out(void *dst, uint64_t dstBytes, const void *p, uint64_t sz, uint64_t *outBytes, hipStream_t stream, uint32_t *errWord = nullptr,
                        const char *errText = nullptr)
    {
        if (outBytes) *outBytes = sz;
        if (!dst) return NRS_OK;
        if (dstBytes < sz) return fail(NRS_E_INVALID, "destination too small");
        if (!sz) return NRS_OK;
        uint32_t e = 0;
        HIPCHK(hipMemcpyAsync(dst, p, sz, hipMemcpyDeviceToHost, stream));
        if (errWord) HIPCHK(hipMemcpyAsync(&e, errWord, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (!e) return NRS_OK;
        HIPCHK(hipMemsetAsync(errWord, 0, 4, stream));
        return fail(NRS_E_STATE, errText);
    }

    // nrs_sample_release, nrs_surface_release, nrs_diffuse_release on sm, sf, df: the stream is drained first, queued work may still use the buffers
    template <typename Part> static int release(Part &part, hipStream_t stream) { HIPCHK(hipStreamSynchronize(stream)); part.release(); return NRS_OK; }

    // ---- field sampling ---------------------------------------------------------------------------------------------------------------
    // the gather: points (device, m of them) or, null, the m nodes of L
    int sample_run(const FluidNow<R> &f, const T4 *points, const Lattice &L, uint64_t m, uint32_t fields)
    {
        const bool walls = (fields & NRS_FIELD_WALLS) && f.bCount;
        GridView<R> G;
        NRSCHK(grid(f, walls, G));
        NRSCHK(sm.ensure_results(fields, m, sizeof(R)));
        const SampleOut<R> O{(fields & NRS_FIELD_DENSITY) ? (R *)sm.result(NRS_FIELD_DENSITY) : nullptr,
                             (fields & NRS_FIELD_GRADIENT) ? (T4 *)sm.result(NRS_FIELD_GRADIENT) : nullptr,
                             (fields & NRS_FIELD_VELOCITY) ? (T4 *)sm.result(NRS_FIELD_VELOCITY) : nullptr,
                             (fields & NRS_FIELD_COUNT) ? (uint32_t *)sm.result(NRS_FIELD_COUNT) : nullptr};
        const dim3 g(nblocks(m)), b(BLOCK);
        const T4 *sP = sm.template sorted_pos<T4>(), *sV = sm.template sorted_vel<T4>();
        if (walls) hipLaunchKernelGGL((k_sample_points<R, KSET, true>), g, b, 0, f.stream, f.P, G, sP, sV, points, L, O, fields, (uint32_t)m);
        else hipLaunchKernelGGL((k_sample_points<R, KSET, false>), g, b, 0, f.stream, f.P, G, sP, sV, points, L, O, fields, (uint32_t)m);
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    // one sample call on m checked queries: points4 (host) or, null, the nodes of L; the result arrays name nothing until it is through
    int sample_queries(const FluidNow<R> &f, const void *points4, const Lattice &L, uint64_t m, uint32_t fields)
    {
        sm.last = SampleLast();
        if (points4 && m) NRSCHK(sm.upload_points(points4, m, sizeof(T4), f.stream));
        if (m) NRSCHK(sample_run(f, points4 ? sm.template query_points<T4>() : nullptr, L, m, fields));
        sm.last = SampleLast{true, fields, m};
        return NRS_OK;
    }
    static int sample_begin(const FluidNow<R> &f, uint32_t fields) { NRSCHK(sample_check_fields(fields)); return sample_refusal(f.facts); }
    int sample_points(const FluidNow<R> &f, const void *points4, uint64_t m, uint32_t fields)
    {
        NRSCHK(sample_begin(f, fields));
        NRSCHK(sample_check_points(points4, m));
        return sample_queries(f, points4, Lattice(), m, fields);
    }
    int sample_lattice(const FluidNow<R> &f, const nrs_lattice *lattice, uint32_t fields)
    {
        NRSCHK(sample_begin(f, fields));
        uint64_t m = 0;
        NRSCHK(sample_check_lattice(lattice, &m));
        return sample_queries(f, nullptr, lattice_from(*lattice), m, fields);
    }
    int sample_device_ptr(uint32_t field, void **dptr, uint64_t *bytes)
    {
        NRSCHK(sample_route_result(sm.last, field, PRECISION, bytes));
        *dptr = *bytes ? sm.result(field) : nullptr;
        return NRS_OK;
    }
    int sample_result(uint32_t field, void *dst, uint64_t dstBytes, uint64_t *outBytes, hipStream_t stream)
    {
        uint64_t sz = 0;
        NRSCHK(sample_route_result(sm.last, field, PRECISION, &sz));
        return copy_out(dst, dstBytes, sm.result(field), sz, outBytes, stream, sm.err_word(),
                        "field sampling: a cell range of the sampler's table lies outside its sorted particles; the gather skipped it, the results are invalid");
    }

    // ---- surface extraction -----------------------------------------------------------------------------------------------------------
    // A sample call on the lattice path (sm's result arrays, refusals and cache rule), then the mesher on sm's result pointers.  The mesh buffers
    // are sf's: no sample call touches them.  iso and flags have passed surface_check_call: the context's state check comes between that and this.
    int surface_extract(const FluidNow<R> &f, const nrs_lattice *lattice, double iso, uint32_t flags, uint64_t *vertices, uint64_t *triangles)
    {
        const uint32_t fields = surface_sample_fields(flags);
        NRSCHK(sample_begin(f, fields));
        uint64_t m = 0;
        NRSCHK(surface_check_lattice(lattice, &m));
        NRSCHK(sample_queries(f, nullptr, lattice_from(*lattice), m, fields));
        const SurfaceInput in{lattice_from(*lattice), m, iso, PRECISION, sm.result(NRS_FIELD_DENSITY),
                              (flags & NRS_SURFACE_GRADIENT) ? sm.result(NRS_FIELD_GRADIENT) : nullptr,
                              (flags & NRS_SURFACE_VELOCITY) ? sm.result(NRS_FIELD_VELOCITY) : nullptr};
        sf.last = SurfaceLast();
        uint64_t V = 0, T = 0;
        NRSCHK(sf.extract(in, f.stream, &V, &T));
        sf.last = SurfaceLast{true, flags, V, T};
        if (vertices) *vertices = V;
        if (triangles) *triangles = T;
        return NRS_OK;
    }
    int surface_device_ptr(uint32_t which, void **dptr, uint64_t *bytes)
    {
        NRSCHK(surface_route_result(sf.last, which, PRECISION, bytes));
        *dptr = *bytes ? sf.result(which) : nullptr;
        return NRS_OK;
    }
    int surface_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes, hipStream_t stream)
    {
        uint64_t sz = 0;
        NRSCHK(surface_route_result(sf.last, which, PRECISION, &sz));
        return copy_out(dst, dstBytes, sf.result(which), sz, outBytes, stream);
    }

    // ---- anisotropic surface reconstruction -----------------------------------------------------------------------------------------------
    // The sampler's particle grid (its cache rule and build count), then pass A on its sorted particles into an's record buffers: recomputed
    // on every call.  cfg has passed aniso_check_config.
    int aniso_records(const FluidNow<R> &f, const AnisoConfig &cfg, GridView<R> &G)
    {
        an.last = AnisoLast();
        NRSCHK(grid(f, false, G));
        NRSCHK(an.template records<R>(f.P, G, cfg, sm.template sorted_pos<T4>(), sm.sorted_index(), sm.sorted_count(), f.stream));
        an.last = AnisoLast{true, sm.sorted_count()};
        return NRS_OK;
    }
    int aniso_build(const FluidNow<R> &f, const nrs_aniso_config *c)
    {
        AnisoConfig cfg;
        NRSCHK(aniso_check_config(c, f.facts.h, &cfg));
        NRSCHK(aniso_refusal(f.facts));
        GridView<R> G;
        return aniso_records(f, cfg, G);
    }
    int aniso_device_ptr(uint32_t which, void **dptr, uint64_t *bytes)
    {
        NRSCHK(aniso_route_result(an.last, which, PRECISION, bytes));
        *dptr = *bytes ? an.result(which) : nullptr;
        return NRS_OK;
    }
    int aniso_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes, hipStream_t stream)
    {
        uint64_t sz = 0;
        NRSCHK(aniso_route_result(an.last, which, PRECISION, &sz));
        return copy_out(dst, dstBytes, an.result(which), sz, outBytes, stream, sm.err_word(),
                        "anisotropic kernels: a cell range of the sampler's table lies outside its sorted particles; the walks skipped it, the results are invalid");
    }
    // Pass A, pass B on the lattice into the sampler's result arrays (sm.last names them: nrs_sample_result afterwards returns the lattice the
    // mesh was cut from), then the mesher as nrs_surface_extract runs it.  iso and flags have passed aniso_check_extract.
    int surface_extract_aniso(const FluidNow<R> &f, const nrs_lattice *lattice, double iso, uint32_t flags, const nrs_aniso_config *c,
                              uint64_t *vertices, uint64_t *triangles)
    {
        const uint32_t fields = aniso_sample_fields(flags);
        AnisoConfig cfg;
        NRSCHK(aniso_check_config(c, f.facts.h, &cfg));
        NRSCHK(aniso_refusal(f.facts));
        uint64_t m = 0;
        NRSCHK(surface_check_lattice(lattice, &m));
        const Lattice L = lattice_from(*lattice);
        GridView<R> G;
        NRSCHK(aniso_records(f, cfg, G));
        sm.last = SampleLast();
        NRSCHK(sm.ensure_results(fields, m, sizeof(R)));
        void *grad = (flags & NRS_SURFACE_GRADIENT) ? sm.result(NRS_FIELD_GRADIENT) : nullptr;
        void *vel = (flags & NRS_SURFACE_VELOCITY) ? sm.result(NRS_FIELD_VELOCITY) : nullptr;
        NRSCHK(an.template lattice<R>(f.P, G, sm.template sorted_vel<T4>(), L, m, sm.result(NRS_FIELD_DENSITY), grad, vel, f.stream));
        sm.last = SampleLast{true, fields, m};
        const SurfaceInput in{L, m, iso, PRECISION, sm.result(NRS_FIELD_DENSITY), grad, vel};
        sf.last = SurfaceLast();
        uint64_t V = 0, T = 0;
        NRSCHK(sf.extract(in, f.stream, &V, &T));
        sf.last = SurfaceLast{true, flags, V, T};
        if (vertices) *vertices = V;
        if (triangles) *triangles = T;
        return NRS_OK;
    }

    // ---- diffuse particles ------------------------------------------------------------------------------------------------------------
    // The sampler's particle grid (its sorted fluid and cell table, its cache rule and build count — its result arrays and `last` are not
    // touched), then the launches of df on its views.  The set's buffers are df's.
    int diffuse_configure(const FluidNow<R> &f, const nrs_diffuse_config *c)
    {
        NRSCHK(diffuse_check_config(c));
        if (f.facts.slab) return fail(NRS_E_INVALID, "diffuse particles on a slab context (its arrays hold halo copies)");
        df.configure(*c);
        return NRS_OK;
    }
    int diffuse_step(const FluidNow<R> &f, double dt)
    {
        NRSCHK(diffuse_check_dt(dt));
        NRSCHK(diffuse_refusal(f.facts, df.last.configured));
        NRSCHK(diffuse_check_births(f.n, df.cfg.max_per_particle));
        GridView<R> G;
        NRSCHK(grid(f, false, G));
        return df.template step<R, KSET>(f.P, G, sm.template sorted_pos<T4>(), sm.template sorted_vel<T4>(), sm.sorted_count(),
                                         dt == 0.0 ? f.P.timestep : (R)dt, f.stream);
    }
    int diffuse_count(hipStream_t stream, uint64_t *alive, uint64_t *byKind, uint64_t *dropped)
    {
        if (!df.last.configured) return fail(NRS_E_STATE, "diffuse particles before nrs_diffuse_configure");
        return df.count(stream, alive, byKind, dropped);
    }
    int diffuse_device_ptr(uint32_t which, void **dptr, uint64_t *bytes, hipStream_t stream)
    {
        NRSCHK(diffuse_route_check(df.last, which));
        uint64_t alive = 0;
        if (!diffuse_per_fluid(which)) NRSCHK(df.alive_now(stream, &alive));
        NRSCHK(diffuse_route_result(df.last, which, alive, PRECISION, bytes));
        *dptr = *bytes ? df.result(which) : nullptr;
        return NRS_OK;
    }
    int diffuse_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes, hipStream_t stream)
    {
        void *p = nullptr;
        uint64_t sz = 0;
        NRSCHK(diffuse_device_ptr(which, &p, &sz, stream));
        // (the word may not exist: an upload can precede any grid build)
        return copy_out(dst, dstBytes, p, sz, outBytes, stream, sm.err_word(),
                        "diffuse particles: a cell range of the sampler's table lies outside its sorted particles; the walks skipped it, the results are invalid");
    }
    int diffuse_upload(const FluidNow<R> &f, const void *pos4, const void *vel4, uint64_t count)
    {
        if (!df.last.configured) {
            if (f.facts.slab) return fail(NRS_E_INVALID, "diffuse particles on a slab context (its arrays hold halo copies)");
            return fail(NRS_E_STATE, "diffuse particles before nrs_diffuse_configure");
        }
        NRSCHK(diffuse_check_upload(pos4, vel4, count, df.cfg.capacity));
        return df.template upload<R>(pos4, vel4, count, f.stream);
    }
};

} // namespace nrs
