// nrs_host_aniso.h — the host decisions of the anisotropic surface reconstruction (include/nereus_hip.h "anisotropic surface
// reconstruction"; DESIGN.md "Anisotropic kernels") and its per-particle finishing routine, written once: which configurations and calls
// are accepted, how many bytes a result takes, which result of the last build an id means; and from the sums of a particle's
// neighbourhood its smoothed centre, the eigen solve of its covariance, the clamps and the record the lattice pass reads.  No HIP: the
// kernels (nrs_kernels_aniso.h) and a plain host program (tests/host_aniso_main.cpp) call the same routine; NRS_ANISO_HD is empty
// without hipcc.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_host_surface.h"

#if defined(__HIPCC__)
#define NRS_ANISO_HD __host__ __device__ inline
#else
#define NRS_ANISO_HD inline
#endif

namespace nrs {

// ---- the configuration ------------------------------------------------------------------------------------------------------------------
// a checked nrs_aniso_config with the defaults filled in; h = interactionRadius
struct AnisoConfig {
    double support, lambda, k_r, k_n, h;
    uint32_t n_eps;
};
// NULL: support = h, lambda = 0.9, k_r = 4, k_n = 0.5, n_eps = 25; a support of 0 means h
static inline int aniso_check_config(const nrs_aniso_config *c, double h, AnisoConfig *out)
{
    AnisoConfig a{h, 0.9, 4.0, 0.5, h, 25u};
    if (c) {
        if (!std::isfinite(c->support) || !std::isfinite(c->lambda) || !std::isfinite(c->k_r) || !std::isfinite(c->k_n))
            return fail(NRS_E_INVALID, "nrs_aniso_config has a non-finite field");
        if (c->reserved) return fail(NRS_E_INVALID, "nrs_aniso_config.reserved must be 0");
        a.support = c->support == 0.0 ? h : c->support;
        a.lambda = c->lambda; a.k_r = c->k_r; a.k_n = c->k_n; a.n_eps = c->n_eps;
    }
    if (!(h > 0.0) || !std::isfinite(h)) return fail(NRS_E_INVALID, "anisotropic kernels need a finite interactionRadius > 0");
    if (!(a.support > 0.0) || !(a.support <= 1.5 * h)) return fail(NRS_E_INVALID, "nrs_aniso_config.support must be in (0, 1.5 h] (0: h)");
    if (!(a.lambda >= 0.0) || !(a.lambda <= 1.0)) return fail(NRS_E_INVALID, "nrs_aniso_config.lambda must be in [0, 1]");
    if (!(a.k_r >= 1.0)) return fail(NRS_E_INVALID, "nrs_aniso_config.k_r must be >= 1");
    if (!(a.k_n > 0.0) || !(a.k_n <= 1.0)) return fail(NRS_E_INVALID, "nrs_aniso_config.k_n must be in (0, 1]");
    if (out) *out = a;
    return NRS_OK;
}
// on top of the sampler's refusals (sample_refusal): a row of the 5 x 5 x 5 walk has five cells
static inline int aniso_refusal(const SampleFacts &f)
{
    NRSCHK(sample_refusal(f));
    for (int a = 0; a < 3; ++a)
        if (f.gridSize[a] < 8u) return fail(NRS_E_INVALID, "anisotropic kernels need gridSize >= 8 on every axis (the five cells of a row alias through the wrap otherwise)");
    return NRS_OK;
}
// nrs_surface_extract_aniso: the mesher's rules, and no wall term
static inline int aniso_check_extract(double iso, uint32_t flags)
{
    NRSCHK(surface_check_call(iso, flags));
    if (flags & NRS_SURFACE_WALLS) return fail(NRS_E_INVALID, "nrs_surface_extract_aniso has no wall term (NRS_SURFACE_WALLS)");
    return NRS_OK;
}
// the NRS_FIELD_* flags the lattice pass writes for the NRS_SURFACE_* flags of an extract
static inline uint32_t aniso_sample_fields(uint32_t flags) { return surface_sample_fields(flags & ~(uint32_t)NRS_SURFACE_WALLS); }

// ---- bytes of a result: `which` is ONE NRS_ANISO_* id, n the particles of the build, precision 32 or 64; 0 for anything else ---------------
static inline uint64_t aniso_result_bytes(uint32_t which, uint64_t n, int precision)
{
    const uint64_t vec4 = precision == 64 ? 32 : 16;
    switch (which) {
    case NRS_ANISO_CENTER: return vec4 * n;
    case NRS_ANISO_G: return 2 * vec4 * n;
    case NRS_ANISO_COUNT: case NRS_ANISO_INDEX: return 4 * n;
    default: return 0;
    }
}
struct AnisoLast {
    bool any = false; // a build has completed since nrs_create / nrs_aniso_release
    uint64_t n = 0;   // its particles
};
static inline int aniso_route_result(const AnisoLast &last, uint32_t which, int precision, uint64_t *bytes)
{
    if (which != NRS_ANISO_CENTER && which != NRS_ANISO_G && which != NRS_ANISO_COUNT && which != NRS_ANISO_INDEX)
        return fail(NRS_E_INVALID, "which must be one of NRS_ANISO_CENTER, _G, _COUNT, _INDEX");
    if (!last.any) return fail(NRS_E_STATE, "no nrs_aniso_build yet (or nrs_aniso_release since)");
    *bytes = aniso_result_bytes(which, last.n, precision);
    return NRS_OK;
}

// ---- the constants of a build in the build's real type --------------------------------------------------------------------------------------
template <typename R> struct AnisoConsts {
    R r, r2;               // neighbourhood radius (R)2 * h and its square
    R k6;                  // 315 / (64 pi r^9): the poly6 constant over r
    R k315;                // 315 / (64 pi)
    R lambda, dmax, amax;  // centre smoothing; largest centre shift h / 2; largest semi-axis 3 h / 2
    R support, k_r, k_n;
    uint32_t n_eps;
};
template <typename R> static inline AnisoConsts<R> aniso_consts(const AnisoConfig &c)
{
    AnisoConsts<R> K;
    const R h = (R)c.h;
    K.r = (R)2 * h;
    K.r2 = K.r * K.r;
    const double pi = 3.14159265358979323846, rd = (double)K.r;
    K.k315 = (R)(315.0 / (64.0 * pi));
    K.k6 = (R)(315.0 / (64.0 * pi * std::pow(rd, 9.0)));
    K.lambda = (R)c.lambda;
    K.dmax = (R)(0.5 * c.h);
    K.amax = (R)(1.5 * c.h);
    K.support = (R)c.support; K.k_r = (R)c.k_r; K.k_n = (R)c.k_n;
    K.n_eps = c.n_eps;
    return K;
}

// ---- the sums of one particle's neighbourhood and the record made from them ------------------------------------------------------------------
template <typename R> struct AnisoSums {
    R sw;                           // sum w
    R mx, my, mz;                   // sum w d
    R sxx, sxy, sxz, syy, syz, szz; // sum w d d^T
    R D;                            // sum (r2 - d2)^3
    uint32_t count;
};
template <typename R> struct AnisoRecord {
    R cx, cy, cz, bound;            // smoothed centre, largest semi-axis
    R g00, g01, g02, g11, g12, g22; // G = U diag(1 / a_k) U^T
    R weight;                       // (315 / (64 pi)) V_i / (a1 a2 a3)
    R a1, a2, a3;                   // the semi-axes, in the eigen solve's order (not stored on the device: the tests read them)
};

NRS_ANISO_HD float aniso_sqrt(float x) { return ::sqrtf(x); }
NRS_ANISO_HD double aniso_sqrt(double x) { return ::sqrt(x); }
NRS_ANISO_HD float aniso_cbrt(float x) { return ::cbrtf(x); }
NRS_ANISO_HD double aniso_cbrt(double x) { return ::cbrt(x); }
NRS_ANISO_HD float aniso_abs(float x) { return ::fabsf(x); }
NRS_ANISO_HD double aniso_abs(double x) { return ::fabs(x); }
template <typename R> NRS_ANISO_HD R aniso_max(R a, R b) { return a < b ? b : a; }
template <typename R> NRS_ANISO_HD R aniso_min(R a, R b) { return b < a ? b : a; }

// One Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q), r the third index: app, aqq, apq the plane's entries, apr and aqr
// the two entries that couple it to r; (v0p, v0q), (v1p, v1q), (v2p, v2q): columns p and q of the accumulated rotations.  The smaller
// root t of t^2 + 2 theta t - 1 = 0 (|t| <= 1); an apq of 0, or a theta whose square overflows, rotates by nothing.
template <typename R>
NRS_ANISO_HD void aniso_rotate(R &app, R &aqq, R &apq, R &apr, R &aqr, R &v0p, R &v0q, R &v1p, R &v1q, R &v2p, R &v2q)
{
    R t = (R)0;
    if (apq != (R)0) {
        const R theta = (aqq - app) / ((R)2 * apq);
        const R den = aniso_abs(theta) + aniso_sqrt(theta * theta + (R)1);
        t = (theta < (R)0 ? (R)-1 : (R)1) / den;
    }
    const R c = (R)1 / aniso_sqrt(t * t + (R)1), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = (R)0;
    const R pr = apr, qr = aqr;
    apr = c * pr - s * qr;
    aqr = s * pr + c * qr;
    R a = v0p, b = v0q;
    v0p = c * a - s * b; v0q = s * a + c * b;
    a = v1p; b = v1q;
    v1p = c * a - s * b; v1q = s * a + c * b;
    a = v2p; b = v2q;
    v2p = c * a - s * b; v2q = s * a + c * b;
}
// sweeps of the cyclic Jacobi: it converges quadratically once the off-diagonal is small, a 3 x 3 matrix is there after three sweeps;
// the count is fixed, so that no trip count depends on the data
template <typename R> struct AnisoSweeps { static constexpr int value = 6; };
template <> struct AnisoSweeps<double> { static constexpr int value = 8; };

// eigenvalues (l0, l1, l2, unordered) and orthonormal eigenvectors (the columns (u00, u10, u20), ...) of the symmetric matrix
// (a00 a01 a02; . a11 a12; . . a22)
template <typename R> struct AnisoEigen { R l0, l1, l2, u00, u01, u02, u10, u11, u12, u20, u21, u22; };
template <typename R> NRS_ANISO_HD AnisoEigen<R> aniso_eigen(R a00, R a01, R a02, R a11, R a12, R a22)
{
    AnisoEigen<R> E;
    E.u00 = E.u11 = E.u22 = (R)1;
    E.u01 = E.u02 = E.u10 = E.u12 = E.u20 = E.u21 = (R)0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < AnisoSweeps<R>::value; ++s) {
        aniso_rotate<R>(a00, a11, a01, a02, a12, E.u00, E.u01, E.u10, E.u11, E.u20, E.u21); // (0, 1), third 2
        aniso_rotate<R>(a00, a22, a02, a01, a12, E.u00, E.u02, E.u10, E.u12, E.u20, E.u22); // (0, 2), third 1
        aniso_rotate<R>(a11, a22, a12, a01, a02, E.u01, E.u02, E.u11, E.u12, E.u21, E.u22); // (1, 2), third 0
    }
    E.l0 = a00; E.l1 = a11; E.l2 = a22;
    return E;
}

// The finishing routine: sums -> centre, covariance, axes, clamps, record.  x: the particle (finite).  A particle without a neighbour
// (count 0: it did not even find itself) or without a volume gets the degenerate record: weight 0, bound 0, G = 0.
template <typename R> NRS_ANISO_HD AnisoRecord<R> aniso_finish(const AnisoConsts<R> &K, R x, R y, R z, const AnisoSums<R> &S)
{
    AnisoRecord<R> O;
    O.cx = x; O.cy = y; O.cz = z;
    O.bound = O.weight = O.g00 = O.g01 = O.g02 = O.g11 = O.g12 = O.g22 = O.a1 = O.a2 = O.a3 = (R)0;
    if (!S.count || !(S.sw > (R)0) || !(S.D > (R)0)) return O;
    // centre
    const R mux = S.mx / S.sw, muy = S.my / S.sw, muz = S.mz / S.sw;
    R dx = K.lambda * mux, dy = K.lambda * muy, dz = K.lambda * muz;
    const R dl = aniso_sqrt((dx * dx + dy * dy) + dz * dz);
    if (dl > K.dmax) {
        const R f = K.dmax / dl;
        dx = dx * f; dy = dy * f; dz = dz * f;
    }
    O.cx = x + dx; O.cy = y + dy; O.cz = z + dz;
    // covariance and its axes
    const R c00 = S.sxx / S.sw - mux * mux, c01 = S.sxy / S.sw - mux * muy, c02 = S.sxz / S.sw - mux * muz;
    const R c11 = S.syy / S.sw - muy * muy, c12 = S.syz / S.sw - muy * muz, c22 = S.szz / S.sw - muz * muz;
    const AnisoEigen<R> E = aniso_eigen<R>(c00, c01, c02, c11, c12, c22);
    const R s1 = aniso_max<R>(E.l0, aniso_max<R>(E.l1, E.l2));
    R a1, a2, a3;
    if (S.count < K.n_eps || !(s1 > (R)0)) {
        a1 = a2 = a3 = K.k_n * K.support;
    } else {
        // (relative to s1: the ratios are in [1 / k_r, 1] and their product cannot underflow; a_k = support * st_k / cbrt(st_1 st_2 st_3))
        const R lo = (R)1 / K.k_r;
        const R t1 = aniso_max<R>(E.l0 / s1, lo), t2 = aniso_max<R>(E.l1 / s1, lo), t3 = aniso_max<R>(E.l2 / s1, lo);
        const R sc = K.support / aniso_cbrt((t1 * t2) * t3);
        a1 = sc * t1; a2 = sc * t2; a3 = sc * t3;
    }
    a1 = aniso_min<R>(a1, K.amax); a2 = aniso_min<R>(a2, K.amax); a3 = aniso_min<R>(a3, K.amax);
    O.a1 = a1; O.a2 = a2; O.a3 = a3;
    const R i1 = (R)1 / a1, i2 = (R)1 / a2, i3 = (R)1 / a3;
    O.g00 = (E.u00 * E.u00 * i1 + E.u01 * E.u01 * i2) + E.u02 * E.u02 * i3;
    O.g01 = (E.u00 * E.u10 * i1 + E.u01 * E.u11 * i2) + E.u02 * E.u12 * i3;
    O.g02 = (E.u00 * E.u20 * i1 + E.u01 * E.u21 * i2) + E.u02 * E.u22 * i3;
    O.g11 = (E.u10 * E.u10 * i1 + E.u11 * E.u11 * i2) + E.u12 * E.u12 * i3;
    O.g12 = (E.u10 * E.u20 * i1 + E.u11 * E.u21 * i2) + E.u12 * E.u22 * i3;
    O.g22 = (E.u20 * E.u20 * i1 + E.u21 * E.u21 * i2) + E.u22 * E.u22 * i3;
    const R V = (R)1 / (K.k6 * S.D);
    O.weight = K.k315 * V / ((a1 * a2) * a3);
    O.bound = aniso_max<R>(a1, aniso_max<R>(a2, a3));
    return O;
}

// ---- one candidate of a neighbourhood (pass A) and of a query (pass B), as the kernels form them -----------------------------------------------
// d = x_j - x_i; true: j is a neighbour and its terms have been added
template <typename R> NRS_ANISO_HD bool aniso_add_neighbour(const AnisoConsts<R> &K, AnisoSums<R> &S, R dx, R dy, R dz)
{
    const R d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 < K.r2)) return false;
    const R q = aniso_sqrt(d2) / K.r;
    const R w = (R)1 - (q * q) * q;
    ++S.count;
    S.sw += w;
    S.mx += w * dx; S.my += w * dy; S.mz += w * dz;
    S.sxx += w * dx * dx; S.sxy += w * dx * dy; S.sxz += w * dx * dz;
    S.syy += w * dy * dy; S.syz += w * dy * dz; S.szz += w * dz * dz;
    const R u = K.r2 - d2;
    S.D += (u * u) * u;
    return true;
}
template <typename R> NRS_ANISO_HD AnisoSums<R> aniso_sums_zero()
{
    AnisoSums<R> S;
    S.sw = S.mx = S.my = S.mz = S.sxx = S.sxy = S.sxz = S.syy = S.syz = S.szz = S.D = (R)0;
    S.count = 0u;
    return S;
}

} // namespace nrs
