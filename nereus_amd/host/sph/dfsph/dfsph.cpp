// dfsph.cpp — Nereus::DFSPH: SPH's update() (upload if dirty, one nrs_step, lazy download) on a context of kind NRS_SOLVER_DFSPH.
#include "dfsph.h"

#include "nereus_hip.h"

#include <cstdio>
#include <cstdlib>

NEREUS_NAMESPACE_BEGIN

DFSPH::DFSPH()
    : SPH(), m_eta(1e-3f), m_etaV(1e-3f), m_akinciGamma(0.0f), m_akinciBeta(0.0f), m_minIters(2), m_minItersV(1), m_warmStart(true), m_viscNu(0.0),
      m_viscNuBoundary(0.0), m_viscTol(1e-3), m_viscMinIters(1), m_viscMaxIters(0)
{
}
DFSPH::DFSPH(SphSimParams params)
    : SPH(params), m_eta(1e-3f), m_etaV(1e-3f), m_akinciGamma(0.0f), m_akinciBeta(0.0f), m_minIters(2), m_minItersV(1), m_warmStart(true),
      m_viscNu(0.0), m_viscNuBoundary(0.0), m_viscTol(1e-3), m_viscMinIters(1), m_viscMaxIters(0)
{
}
DFSPH::~DFSPH() {}

int DFSPH::solverKind() const { return NRS_SOLVER_DFSPH; }

void DFSPH::setSolverSettings(SReal eta, SUint minIters, SReal etaV, SUint minItersV, bool warmStart)
{
    if (m_ctx) { // (a context keeps the settings it was created with)
        std::fprintf(stderr, "Nereus: DFSPH::setSolverSettings must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_eta = eta;
    m_minIters = minIters;
    m_etaV = etaV;
    m_minItersV = minItersV;
    m_warmStart = warmStart;
}

void DFSPH::setAkinciSurface(SReal gamma, SReal beta)
{
    if (m_ctx) {
        std::fprintf(stderr, "Nereus: DFSPH::setAkinciSurface must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_akinciGamma = gamma;
    m_akinciBeta = beta;
}

void DFSPH::setImplicitViscosity(double nu, double nuBoundary, double tol, SUint minIters, SUint maxIters)
{
    m_viscNu = nu;
    m_viscNuBoundary = nuBoundary;
    m_viscTol = tol;
    m_viscMinIters = minIters;
    m_viscMaxIters = maxIters;
    if (m_ctx && nrs_dfsph_set_viscosity(m_ctx, nu, nuBoundary, tol, (uint32_t)minIters, (uint32_t)maxIters) != NRS_OK)
        fatal("nrs_dfsph_set_viscosity");
}

bool DFSPH::implicitViscosityInfo(SUint *iterations, double *residual, double *rhsNorm)
{
    uint32_t it = 0;
    int on = 0;
    if (!m_ctx || nrs_dfsph_viscosity_info(m_ctx, &on, &it, residual, rhsNorm) != NRS_OK) return false;
    if (iterations) *iterations = (SUint)it;
    return on != 0;
}

void DFSPH::configureContext()
{
    if (nrs_dfsph_configure(m_ctx, (double)m_eta, (uint32_t)m_minIters, (double)m_etaV, (uint32_t)m_minItersV, m_warmStart ? 1 : 0) != NRS_OK)
        fatal("nrs_dfsph_configure");
    if (nrs_set_surface_akinci(m_ctx, (double)m_akinciGamma, (double)m_akinciBeta) != NRS_OK) fatal("nrs_set_surface_akinci");
    if (nrs_dfsph_set_viscosity(m_ctx, m_viscNu, m_viscNuBoundary, m_viscTol, (uint32_t)m_viscMinIters,
                                (uint32_t)m_viscMaxIters) != NRS_OK)
        fatal("nrs_dfsph_set_viscosity");
}

SUint DFSPH::getLastIterations()
{
    uint32_t it = 0;
    if (m_ctx && nrs_last_iterations(m_ctx, &it) != NRS_OK) fatal("nrs_last_iterations");
    return (SUint)it;
}

NEREUS_NAMESPACE_END
