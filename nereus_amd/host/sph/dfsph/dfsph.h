// dfsph.h — Nereus::DFSPH, divergence-free SPH (Bender & Koschier 2015 / 2017).  Not in the reference: a device step of the library's
// NRS_SOLVER_DFSPH (DESIGN.md "DFSPH") behind the SPH host surface.  update() is a full step; the pressures read back are the step's
// K (m^2), the density solve's warm-start total.
//
// Checkpoints: saveState() / loadState() carry K as the pressure, so a restored run warm-starts its density solve as the original
// did; the divergence solve's total Kv is not in the checkpoint and restarts at zero.  A restored run is therefore bit-identical to
// the original only with the divergence warm start off (warmStart = false, or the divergence solve off).  The checkpoint format is
// unchanged.
#pragma once
#ifndef DFSPH_H
#define DFSPH_H
#include "sph.h"

NEREUS_NAMESPACE_BEGIN

class DFSPH : public SPH {
public:
    DFSPH();
    DFSPH(SphSimParams params);
    virtual ~DFSPH();
    // Solver settings (nrs_dfsph_configure).  Must be called before the device context exists, i.e. before the first update() or
    // updateGpuBoundaries().  eta / etaV = the average error each loop accepts (0: exactly minIters / minItersV iterations, nothing
    // read back), minItersV = 0 turns the divergence solve off, warmStart = start both solves from half the previous step's totals.
    // Defaults 1e-3, 2, 1e-3, 1, true.
    void setSolverSettings(SReal eta, SUint minIters, SReal etaV, SUint minItersV, bool warmStart);
    // Surface tension gamma and wall adhesion beta of Akinci et al. 2013 (nrs_set_surface_akinci; 0, 0: off).  Same rule as
    // setSolverSettings: before the context exists.
    void setAkinciSurface(SReal gamma, SReal beta);
    // The implicit viscosity solve (nrs_dfsph_set_viscosity, DESIGN.md "Implicit viscosity"): behind the advection launch the step solves
    // (I - dt nu L) u = v* by conjugate gradients.  nu: the kinematic viscosity in m^2/s (0: off, the default), nuBoundary: the friction
    // against walls at rest (0: slip; not together with moving boundary bodies), tol: the relative residual the solve stops at (0: exactly
    // minIters iterations, nothing read back), maxIters: the cap (0 = 100).  The explicit viscous term keeps obeying the parameters'
    // viscosity: set that to 0 for the implicit term alone.  May be called at any time; a context that exists takes the settings at once.
    void setImplicitViscosity(double nu, double nuBoundary, double tol, SUint minIters, SUint maxIters);
    // What the last step's solve left (nrs_dfsph_viscosity_info): false while the solve is off or before its first step
    bool implicitViscosityInfo(SUint *iterations, double *residual, double *rhsNorm);
    SUint getLastIterations(); // density-solve iterations of the last step
    int solverKind() const override;

protected:
    void configureContext() override; // hands the settings to every context ensureContext creates (a capacity change replaces it)
    SReal m_eta, m_etaV;
    SReal m_akinciGamma, m_akinciBeta;
    SUint m_minIters, m_minItersV;
    bool m_warmStart;
    double m_viscNu, m_viscNuBoundary, m_viscTol; // (as given: the ABI takes doubles)
    SUint m_viscMinIters, m_viscMaxIters;
};

NEREUS_NAMESPACE_END
#endif // DFSPH_H
