// pbf.h — Nereus::PBF, position-based fluids (Macklin & Mueller 2013).  Not in the reference, which names PBF among its future works:
// a device step of the library's NRS_SOLVER_PBF (DESIGN.md "PBF") behind the SPH host surface.  update() is a full step; the
// pressures read back are the step's lambda.
#pragma once
#ifndef PBF_H
#define PBF_H
#include "sph.h"

NEREUS_NAMESPACE_BEGIN

class PBF : public SPH {
public:
    PBF();
    PBF(SphSimParams params);
    virtual ~PBF();
    // Solver settings (nrs_pbf_configure).  Must be called before the device context exists, i.e. before the first update() or
    // updateGpuBoundaries().  eta = largest density error max(rho - rho0, 0) / rho0 the loop accepts (0: exactly minIters iterations,
    // nothing read back), relaxation = eps / D_proto, xsph = the XSPH velocity smoothing factor (0 = off).
    void setSolverSettings(SReal eta, SUint minIters, SReal relaxation, SReal xsph);
    // Tensile correction s_corr = -k (W / W((dq h, 0, 0)))^4 on fluid pairs (nrs_pbf_set_tensile; k = 0: off) and vorticity
    // confinement with factor eps (nrs_pbf_set_vorticity; 0: off).  Same rule as setSolverSettings: before the context exists.
    void setTensileCorrection(SReal k, SReal dq);
    void setVorticityConfinement(SReal eps);
    // Surface tension gamma and wall adhesion beta of Akinci et al. 2013 (nrs_set_surface_akinci; 0, 0: off).  Same rule as
    // setSolverSettings: before the context exists.
    void setAkinciSurface(SReal gamma, SReal beta);
    SUint getLastIterations(); // solver iterations of the last step
    int solverKind() const override;

protected:
    void configureContext() override; // hands the settings to every context ensureContext creates (a capacity change replaces it)
    SReal m_eta, m_relaxation, m_xsph;
    SReal m_tensileK, m_tensileDq, m_vorticity;
    SReal m_akinciGamma, m_akinciBeta;
    SUint m_minIters;
};

NEREUS_NAMESPACE_END
#endif // PBF_H
