// pcisph.cpp — Nereus::PCISPH as the reference leaves it (sph/pcisph/pcisph.cpp:161-204): update() uploads the host state,
// builds the neighbour grid (calcHash / sortParticles / reorderDataAndFindCellStart), evaluates density and Tait pressure
// (pcisph_internalForces launches computeDensityPressure, sph_cuda.cu:905-936), runs the EMPTY pressure solve
// (pcisph_pressureSolve, sph_cuda.cu:944-952) and copies the SORTED positions / velocities back to the host arrays
// (:201-202): nothing moves, but the host arrays come back permuted into hash order.  Mirrored here exactly;
// densities and pressures of the step are additionally readable on the host (getHostDensity / getHostPressure).
// setPressureSolve(true) replaces the stub with the library's PCISPH step (a context of kind NRS_SOLVER_PCISPH).
#include "pcisph.h"

#include "nereus_hip.h"

#include <cstdio>
#include <cstdlib>

NEREUS_NAMESPACE_BEGIN

PCISPH::PCISPH() : SPH(), m_pressureSolve(false), m_eta(0.01f), m_akinciGamma(0.0f), m_akinciBeta(0.0f) {}
PCISPH::PCISPH(SphSimParams params) : SPH(params), m_pressureSolve(false), m_eta(0.01f), m_akinciGamma(0.0f), m_akinciBeta(0.0f) {}
PCISPH::~PCISPH() {}
void PCISPH::_initialize() { SPH::_initialize(); }
void PCISPH::_finalize() { SPH::_finalize(); }

int PCISPH::solverKind() const { return m_pressureSolve ? NRS_SOLVER_PCISPH : NRS_SOLVER_SESPH; }

void PCISPH::setPressureSolve(bool on, SReal eta)
{
    if (m_ctx) { // (the context's kind is fixed when it is created)
        std::fprintf(stderr, "Nereus: PCISPH::setPressureSolve must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_pressureSolve = on;
    m_eta = eta;
}

void PCISPH::setAkinciSurface(SReal gamma, SReal beta)
{
    if (m_ctx) {
        std::fprintf(stderr, "Nereus: PCISPH::setAkinciSurface must be called before the first update() / updateGpuBoundaries()\n");
        std::exit(EXIT_FAILURE);
    }
    m_akinciGamma = gamma;
    m_akinciBeta = beta;
}

void PCISPH::configureContext()
{
    if (!m_pressureSolve) return;
    if (nrs_pcisph_configure(m_ctx, (double)m_eta, 3, 0.0, 0.0) != NRS_OK) fatal("nrs_pcisph_configure");
    if (nrs_set_surface_akinci(m_ctx, (double)m_akinciGamma, (double)m_akinciBeta) != NRS_OK) fatal("nrs_set_surface_akinci");
}

SUint PCISPH::getLastIterations()
{
    uint32_t it = 0;
    if (m_pressureSolve && m_ctx && nrs_last_iterations(m_ctx, &it) != NRS_OK) fatal("nrs_last_iterations");
    return (SUint)it;
}

void PCISPH::update()
{
    if (m_numParticles == 0) return;
    if (m_pressureSolve) {
        SPH::update(); // upload if dirty → step → lazy download (pressures included)
        return;
    }
    ensureContext();
    m_hostDirty = true; // the reference uploads the host arrays every step (pcisph.cpp:164-165)
    pushHostToDevice();
    if (nrs_set_params(m_ctx, &m_params) != NRS_OK) fatal("nrs_set_params");
    if (nrs_step_partial(m_ctx, NRS_STAGE_DENSITY) != NRS_OK) fatal("nrs_step_partial");
    // D2H of the sorted arrays (pcisph.cpp:201-202) + the step's density / pressure
    const uint64_t v = sizeof(SReal) * 4 * (uint64_t)m_numParticles, sc = sizeof(SReal) * (uint64_t)m_numParticles;
    if (nrs_get_array(m_ctx, NRS_ARR_SORTED_POS, m_pos, v, nullptr) != NRS_OK) fatal("nrs_get_array(sorted pos)");
    if (nrs_get_array(m_ctx, NRS_ARR_SORTED_VEL, m_vel, v, nullptr) != NRS_OK) fatal("nrs_get_array(sorted vel)");
    if (nrs_get_array(m_ctx, NRS_ARR_DENS, m_density, sc, nullptr) != NRS_OK) fatal("nrs_get_array(dens)");
    if (nrs_get_array(m_ctx, NRS_ARR_PRES, m_pressure, sc, nullptr) != NRS_OK) fatal("nrs_get_array(pres)");
    m_deviceNewer = false; // the host arrays are the state now (the partial step left the device mid-update)
    m_hostDirty = true;
}

NEREUS_NAMESPACE_END
