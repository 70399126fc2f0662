// pbf.cpp — Nereus::PBF: SPH's update() (upload if dirty, one nrs_step, lazy download) on a context of kind NRS_SOLVER_PBF.
#include "pbf.h"

#include "nereus_hip.h"

#include <cstdio>
#include <cstdlib>

NEREUS_NAMESPACE_BEGIN

PBF::PBF()
    : SPH(), m_eta(0.01f), m_relaxation(0.01f), m_xsph(0.0f), m_tensileK(0.0f), m_tensileDq(0.2f), m_vorticity(0.0f), m_akinciGamma(0.0f),
      m_akinciBeta(0.0f), m_minIters(2)
{
}
PBF::PBF(SphSimParams params)
    : SPH(params), m_eta(0.01f), m_relaxation(0.01f), m_xsph(0.0f), m_tensileK(0.0f), m_tensileDq(0.2f), m_vorticity(0.0f), m_akinciGamma(0.0f),
      m_akinciBeta(0.0f), m_minIters(2)
{
}
PBF::~PBF() {}

int PBF::solverKind() const { return NRS_SOLVER_PBF; }

void PBF::setSolverSettings(SReal eta, SUint minIters, SReal relaxation, SReal xsph)
{
    if (m_ctx) { // (a context keeps the settings it was created with)
        std::fprintf(stderr, "Nereus: PBF::setSolverSettings must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_eta = eta;
    m_minIters = minIters;
    m_relaxation = relaxation;
    m_xsph = xsph;
}

void PBF::setTensileCorrection(SReal k, SReal dq)
{
    if (m_ctx) {
        std::fprintf(stderr, "Nereus: PBF::setTensileCorrection must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_tensileK = k;
    m_tensileDq = dq;
}

void PBF::setVorticityConfinement(SReal eps)
{
    if (m_ctx) {
        std::fprintf(stderr, "Nereus: PBF::setVorticityConfinement must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_vorticity = eps;
}

void PBF::setAkinciSurface(SReal gamma, SReal beta)
{
    if (m_ctx) {
        std::fprintf(stderr, "Nereus: PBF::setAkinciSurface must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_akinciGamma = gamma;
    m_akinciBeta = beta;
}

void PBF::configureContext()
{
    if (nrs_pbf_configure(m_ctx, (double)m_eta, (uint32_t)m_minIters, (double)m_relaxation, (double)m_xsph) != NRS_OK)
        fatal("nrs_pbf_configure");
    if (nrs_pbf_set_tensile(m_ctx, (double)m_tensileK, (double)m_tensileDq) != NRS_OK) fatal("nrs_pbf_set_tensile");
    if (nrs_pbf_set_vorticity(m_ctx, (double)m_vorticity) != NRS_OK) fatal("nrs_pbf_set_vorticity");
    if (nrs_set_surface_akinci(m_ctx, (double)m_akinciGamma, (double)m_akinciBeta) != NRS_OK) fatal("nrs_set_surface_akinci");
}

SUint PBF::getLastIterations()
{
    uint32_t it = 0;
    if (m_ctx && nrs_last_iterations(m_ctx, &it) != NRS_OK) fatal("nrs_last_iterations");
    return (SUint)it;
}

NEREUS_NAMESPACE_END
