// nrs_host_viscosity.h — the host decisions of the implicit viscosity solve of the DFSPH step (DESIGN.md "Implicit viscosity"): the
// settings of nrs_dfsph_set_viscosity with their checks, the inputs of the exit rule, the sizes of the solve's buffers, the layout of
// its device scalars, and the guards of the two CG coefficients as plain functions that the kernels call too.  No HIP.
//
// The solve: after the advection launch, (I - dt nu L) u = v* by plain conjugate gradients, u0 = b = v* = vel_adv, r0 = p0 = b - A b;
// per iteration q = A p, alpha = rr / (p.q), u += alpha p, r -= alpha q, beta = rr' / rr, p = r + beta p.  The result replaces vel_adv.
// The explicit viscous term of the advection launch keeps obeying params.viscosity: set that to 0 for the implicit term alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "nrs_error.h"

#if defined(__HIPCC__)
#define NRS_VISC_HD __host__ __device__ inline
#else
#define NRS_VISC_HD inline
#endif

namespace nrs {

constexpr uint32_t VISC_DEFAULT_CAP = 100; // max_iters = 0

struct ViscSettings { // nrs_dfsph_set_viscosity; nu = 0: off
    double nu = 0.0, nuB = 0.0, tol = 0.0;
    uint32_t minIters = 0, maxIters = 0;
    bool on() const { return nu > 0.0; }
    // movingBodies: the context's boundary particles are grouped into moving bodies (wall friction would need the wall's velocity on the
    // right-hand side)
    int set(double nu_, double nuB_, double tol_, uint32_t minIters_, uint32_t maxIters_, bool movingBodies)
    {
        if (!std::isfinite(nu_) || nu_ < 0.0 || !std::isfinite(nuB_) || nuB_ < 0.0)
            return fail(NRS_E_INVALID, "implicit viscosity: nu and nu_boundary must be finite and >= 0");
        if (!(tol_ >= 0.0 && tol_ < 1.0)) return fail(NRS_E_INVALID, "implicit viscosity: tolerance must be in [0, 1)");
        if (tol_ == 0.0 && minIters_ == 0) return fail(NRS_E_INVALID, "implicit viscosity: tolerance 0 (a fixed count) needs min_iters >= 1");
        if (maxIters_ != 0 && maxIters_ < minIters_) return fail(NRS_E_INVALID, "implicit viscosity: max_iters below min_iters (0 = 100)");
        if (nu_ > 0.0 && nuB_ > 0.0 && movingBodies)
            return fail(NRS_E_STATE, "implicit viscosity: wall friction (nu_boundary > 0) on a context whose boundary bodies move");
        nu = nu_; nuB = nu_ > 0.0 ? nuB_ : 0.0; tol = tol_; minIters = minIters_; maxIters = maxIters_;
        return NRS_OK;
    }
    // the inputs of solve_loop (nrs_host_plan.h): fixed mode runs exactly min_iters iterations and reads nothing back
    bool fixed() const { return tol == 0.0; }
    uint32_t cap() const { return fixed() ? minIters : (maxIters ? maxIters : VISC_DEFAULT_CAP); }
    // rr <= tol^2 bb, as a measure against the threshold 0: solve_loop stops on measure <= eta
    double measure(double rr, double bb) const { return rr - tol * tol * bb; }
};

// the solve's device scalars, doubles: |b|^2, p.q, the two slots rr alternates between (the iteration's rr and the next one's), and
// the count of iterations that began with rr > 0
enum { VISC_BB = 0, VISC_PQ = 1, VISC_RR0 = 2, VISC_RR1 = 3, VISC_ITERS = 4, VISC_SCALARS = 8 };
inline int visc_rr_slot(uint32_t iteration) { return (iteration & 1u) ? VISC_RR1 : VISC_RR0; } // the slot that holds rr when `iteration` starts

// the buffers: r, p, q as vec4 per particle of the capacity, two per-particle dot terms, the scalars
struct ViscBufferSizes { size_t vec, dots, scalars; };
inline ViscBufferSizes visc_buffer_sizes(uint64_t capacity, size_t realBytes)
{
    return ViscBufferSizes{(size_t)capacity * 4 * realBytes, (size_t)capacity * realBytes, VISC_SCALARS * sizeof(double)};
}

// the CG coefficients from the reduced sums: alpha = 0 when p.q <= 0 (or not a number), beta = 0 when rr = 0
NRS_VISC_HD double visc_alpha(double rr, double pq) { return pq > 0.0 ? rr / pq : 0.0; }
NRS_VISC_HD double visc_beta(double rrNew, double rr) { return rr > 0.0 ? rrNew / rr : 0.0; }

} // namespace nrs
