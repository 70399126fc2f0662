// nrs_viscosity.h — the owner of the implicit viscosity solve of the DFSPH step (DESIGN.md "Implicit viscosity"): its settings
// (nrs_host_viscosity.h), its buffers — r, p, q, the per-particle dot terms and the device scalars, none of which exists before the first
// configure with nu > 0 — the CG loop and what the last solve left for nrs_dfsph_viscosity_info.  It carries nothing from step to
// step and nothing of it follows the sort.  The context holds one next to its PressureSolvers (nrs_solvers.h), whose pci_prefix calls
// solve() behind the advection launch of a DFSPH step and hands it the one thing that depends on the kernel set and the walls: the
// launch of the matvec pass.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_plan.h"
#include "nrs_host_viscosity.h"
#include "nrs_kernels_viscosity.h"

namespace nrs {

template <typename R> struct ViscositySolver {
    typedef typename Vec4T<R>::type T4;
    bool on() const { return s.on(); }
    bool wall_friction() const { return s.on() && s.nuB > 0.0; }

    // nrs_dfsph_set_viscosity, after the refusal of a context that is not DFSPH.  nu = 0: off, and the buffers go.
    int configure(uint64_t capacity, double nu, double nuB, double tol, uint32_t minIters, uint32_t maxIters, bool movingBodies)
    {
        ViscSettings t;
        NRSCHK(t.set(nu, nuB, tol, minIters, maxIters, movingBodies));
        if (t.on()) {
            const ViscBufferSizes z = visc_buffer_sizes(capacity, sizeof(R));
            NRSCHK(r.alloc(z.vec));
            NRSCHK(p.alloc(z.vec));
            NRSCHK(q.alloc(z.vec));
            NRSCHK(dotA.alloc(z.dots));
            NRSCHK(dotB.alloc(z.dots));
            NRSCHK(scal.alloc(z.scalars));
        } else {
            r.release(); p.release(); q.release(); dotA.release(); dotB.release(); scal.release();
        }
        s = t;
        solved = false;
        return NRS_OK;
    }

    // (I - dt nu L) u = b in place on u = b = vel_adv.  matvec(start, A): one launch of ViscMatvecPass<R, KSET, start> with the arrays A.
    template <typename Reduce, typename Matvec>
    int solve(Reduce &red, const Params<R> &P, T4 *u, const R *dens, uint32_t N, hipStream_t stream, Matvec &&matvec)
    {
        const dim3 g(nblocks(N)), b(BLOCK);
        double *sc = scal.as<double>();
        ViscArrays<R> A;
        A.in = u; A.dens = dens; A.r = r.as<T4>(); A.p = p.as<T4>(); A.q = q.as<T4>(); A.dotA = dotA.as<R>(); A.dotB = dotB.as<R>();
        A.cF = (R)(10.0 * (double)P.timestep * s.nu);
        A.cB = (R)(10.0 * (double)P.timestep * s.nuB);
        HIPCHK(hipMemsetAsync(sc, 0, scal.bytes, stream));
        matvec(std::true_type{}, A);
        red.sum_to(A.dotA, N, sc + visc_rr_slot(0));
        red.sum_to(A.dotB, N, sc + VISC_BB);
        A.in = A.p;
        double h[VISC_SCALARS];
        double m = 0.0;
        uint32_t done = 0;
        NRSCHK(solve_loop(
            s.fixed(), s.minIters, s.cap(), 0.0,
            [&](uint32_t k) {
                const int cur = visc_rr_slot(k), next = visc_rr_slot(k + 1);
                matvec(std::false_type{}, A);
                red.sum_to(A.dotA, N, sc + VISC_PQ);
                hipLaunchKernelGGL((k_visc_update<R>), g, b, 0, stream, sc, cur, u, A.r, (const T4 *)A.p, (const T4 *)A.q, A.dotA, N);
                red.sum_to(A.dotA, N, sc + next);
                hipLaunchKernelGGL((k_visc_direction<R>), g, b, 0, stream, (const double *)sc, cur, next, A.p, (const T4 *)A.r, N);
                done = k + 1;
            },
            [&](double *e) { // the exit test's one read-back: rr of the iteration just queued, and |b|^2
                HIPCHK(hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                *e = s.measure(h[visc_rr_slot(done)], h[VISC_BB]);
                return (int)NRS_OK;
            },
            &queued, &m));
        HIPCHK(hipGetLastError()); // (a launch that failed above, as in the other chains)
        solved = true;
        return NRS_OK;
    }

    // nrs_dfsph_viscosity_info: read from the device scalars on request; waits for the stream
    int info(hipStream_t stream, int *isOn, uint32_t *iterations, double *residual, double *rhsNorm)
    {
        if (isOn) *isOn = on() ? 1 : 0;
        if (!on() || !solved) return fail(NRS_E_STATE, "nrs_dfsph_viscosity_info before a step with the implicit viscosity solve on");
        double h[VISC_SCALARS];
        HIPCHK(hipMemcpyAsync(h, scal.p, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (iterations) *iterations = (uint32_t)h[VISC_ITERS];
        if (residual) *residual = std::sqrt(h[visc_rr_slot(queued)]);
        if (rhsNorm) *rhsNorm = std::sqrt(h[VISC_BB]);
        return NRS_OK;
    }

private:
    ViscSettings s;
    DevBuf r, p, q, dotA, dotB, scal;
    uint32_t queued = 0; // iterations the last solve queued: its last rr is in visc_rr_slot(queued)
    bool solved = false; // a step has run the solve since the last configure
};

} // namespace nrs
