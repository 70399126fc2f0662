// nrs_host_settings.h — the caller-given settings of the PCISPH, PBF and DFSPH solvers and of the Akinci surface model, as given (double
// / uint32_t), with their defaults and their argument validation.  No HIP.  What the context derives from them in SReal (delta, eps,
// W_q, the DFSPH threshold), the flags that say those belong to the current parameters, and the refusal of a call on a context of
// another solver stay in the context (nrs_ctx_impl.h).  Every set validates first and stores only what passed; where the context has
// device work to do that may fail (a buffer, W_q), it sets a copy and keeps it once that work is done.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_error.h"

namespace nrs {

struct PciSettings { // nrs_pcisph_configure
    double eta = 0.01, spacing = 0.0, deltaGiven = 0.0;
    uint32_t minIters = 3;
    int set(double eta_, uint32_t minIters_, double spacing_, double delta_)
    {
        if (!(eta_ > 0.0) || !std::isfinite(eta_)) return fail(NRS_E_INVALID, "max_density_error must be > 0");
        if (minIters_ == 0) return fail(NRS_E_INVALID, "min_iters must be >= 1");
        if (!(spacing_ >= 0.0) || !std::isfinite(spacing_)) return fail(NRS_E_INVALID, "prototype_spacing must be >= 0 (0 = cbrt(m / rho0))");
        if (!(delta_ >= 0.0) || !std::isfinite(delta_)) return fail(NRS_E_INVALID, "delta must be >= 0 (0 = from the prototype)");
        eta = eta_; minIters = minIters_; spacing = spacing_; deltaGiven = delta_;
        return NRS_OK;
    }
};

struct PbfSettings { // nrs_pbf_configure, nrs_pbf_set_tensile (k = 0: off), nrs_pbf_set_vorticity (eps_v = 0: off)
    double eta = 0.01, relax = 0.01, xsph = 0.0;
    uint32_t minIters = 2;
    double tensK = 0.0, tensDq = 0.2, vortEps = 0.0;
    int set(double eta_, uint32_t minIters_, double relaxation, double xsph_)
    {
        if (!(eta_ >= 0.0) || !std::isfinite(eta_)) return fail(NRS_E_INVALID, "max_density_error must be >= 0 (0 = a fixed min_iters iterations)");
        if (minIters_ == 0) return fail(NRS_E_INVALID, "min_iters must be >= 1");
        if (!(relaxation > 0.0) || !std::isfinite(relaxation)) return fail(NRS_E_INVALID, "relaxation must be > 0");
        if (!(xsph_ >= 0.0 && xsph_ <= 1.0)) return fail(NRS_E_INVALID, "xsph must be in [0, 1]");
        eta = eta_; minIters = minIters_; relax = relaxation; xsph = xsph_;
        return NRS_OK;
    }
    int set_tensile(double k, double dq)
    {
        if (!(k >= 0.0) || !std::isfinite(k)) return fail(NRS_E_INVALID, "tensile k must be finite and >= 0 (0 = off)");
        if (!(dq > 0.0 && dq < 1.0)) return fail(NRS_E_INVALID, "tensile dq must be in (0, 1)");
        tensK = k; tensDq = dq;
        return NRS_OK;
    }
    int set_vorticity(double epsV)
    {
        if (!(epsV >= 0.0) || !std::isfinite(epsV)) return fail(NRS_E_INVALID, "vorticity eps_v must be finite and >= 0 (0 = off)");
        vortEps = epsV;
        return NRS_OK;
    }
};

struct DfsphSettings { // nrs_dfsph_configure
    double eta = 1e-3, etaV = 1e-3;
    uint32_t minIters = 2, minItersV = 1;
    bool warm = true;
    int set(double eta_, uint32_t minIters_, double etaV_, uint32_t minItersV_, int warm_)
    {
        if (!std::isfinite(eta_) || eta_ < 0.0 || !std::isfinite(etaV_) || etaV_ < 0.0)
            return fail(NRS_E_INVALID, "DFSPH: max_density_error and max_divergence_error must be finite and >= 0");
        if (minIters_ == 0) return fail(NRS_E_INVALID, "DFSPH: min_iters must be >= 1");
        if (warm_ != 0 && warm_ != 1) return fail(NRS_E_INVALID, "DFSPH: warm_start must be 0 or 1");
        eta = eta_; minIters = minIters_; etaV = etaV_; minItersV = minItersV_; warm = warm_ != 0;
        return NRS_OK;
    }
};

struct AkinciSettings { // nrs_set_surface_akinci: gamma = beta = 0 is off
    double gamma = 0.0, beta = 0.0;
    int set(double gamma_, double beta_)
    {
        if (!(gamma_ >= 0.0) || !std::isfinite(gamma_)) return fail(NRS_E_INVALID, "Akinci gamma must be finite and >= 0 (0 = off)");
        if (!(beta_ >= 0.0) || !std::isfinite(beta_)) return fail(NRS_E_INVALID, "Akinci beta_adhesion must be finite and >= 0 (0 = off)");
        gamma = gamma_; beta = beta_;
        return NRS_OK;
    }
};

} // namespace nrs
