// pcisph.h — Nereus::PCISPH.  The reference's PCISPH is unfinished (README "soon finished"): its update()
// computes densities and its pressure solve is an empty stub (sph/pcisph/pcisph.cpp:161-204,
// sph_kernel_impl.cuh:1722-1730).  This header exists so main.cpp:6 still includes; the class behaves like
// the reference's: a step evaluates density/pressure and moves nothing.  setPressureSolve(true) opts in to the library's
// predictive-corrective solver (NRS_SOLVER_PCISPH, DESIGN.md "PCISPH"): update() is then a full device step.
#pragma once
#ifndef PCISPH_H
#define PCISPH_H
#include "sph.h"

NEREUS_NAMESPACE_BEGIN

class PCISPH : public SPH {
public:
    PCISPH();
    PCISPH(SphSimParams params);
    virtual ~PCISPH();
    virtual void _initialize();
    virtual void _finalize();
    void update();
    // Opt in to the PCISPH pressure solve (off: the reference's stub).  Must be called before the device context exists, i.e.
    // before the first update() or updateGpuBoundaries(); eta = largest density error max(rho - rho0, 0) / rho0 the loop accepts.
    void setPressureSolve(bool on, SReal eta = 0.01f);
    // Surface tension gamma and wall adhesion beta of Akinci et al. 2013 (nrs_set_surface_akinci; 0, 0: off) for the opted-in pressure
    // solve (the stub ignores them).  Same rule as setPressureSolve: before the context exists.
    void setAkinciSurface(SReal gamma, SReal beta);
    SUint getLastIterations(); // solver iterations of the last step (0 for the stub)
    virtual int solverKind() const;

protected:
    virtual void configureContext(); // hands eta to every context ensureContext creates (a capacity change replaces it)
    bool m_pressureSolve;
    SReal m_eta;
    SReal m_akinciGamma, m_akinciBeta;
};

NEREUS_NAMESPACE_END
#endif // PCISPH_H
