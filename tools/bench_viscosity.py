"""The implicit viscosity solve of the DFSPH step at config C3 (160^3 = 4,096,000 particles, fp32, Muller, IISPH constructor parameters,
dam break with the boundary box; tools/bench_dfsph.py's scene).  Per run a short untimed spin-up, then `--steps` steps with the stages
timed by device events (nrs_stage_ms).  DFSPH runs in fixed-count mode without warm start, so that the stage times are linear in the
counts:

  * ms per CG iteration: the difference of NRS_STAGE_P_ADVECT between a fixed `--hi` and a fixed `--lo` CG iterations, per iteration;
  * the yardstick of the same process: ms per DFSPH A+B pair, the difference of NRS_STAGE_P_SOLVE between `--hi` and `--lo` density
    iterations, per iteration;
  * launches per CG iteration (the matvec, the two launches of each of the two sums, the two vector kernels);
  * the CG iterations to tolerance 1e-3 for nu = 0.01, 1 and 100 (the mean over the timed steps, and |r| / |b| of the last).

Prints one JSON line.

    python tools/bench_viscosity.py [--steps 10] [--spin-up 3] [--lo 2] [--hi 10] [--config C3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nereus_amd import capi, scene  # noqa: E402
from nereus_amd.params import default_params  # noqa: E402

LAUNCHES_PER_ITERATION = 7


def run(sc, p, steps, spin_up, density_iters, visc):
    """stage ms per step of a DFSPH run with `density_iters` fixed density iterations and the viscosity settings `visc` (None: off)"""
    stream = torch.cuda.current_stream()
    s = capi.Solver(p, len(sc["pos"]), solver=capi.DFSPH, device=0, stream=stream.cuda_stream)
    s.dfsph_configure(0.0, density_iters, 0.0, 1, False)
    if visc is not None:
        s.dfsph_set_viscosity(*visc)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(spin_up):
        s.step(1)
    s.synchronize()
    s.set_profiling(True)
    iters = []
    info = None
    for _ in range(steps):
        s.step(1)
        if visc is not None and visc[2] > 0.0:   # (tolerance mode waits anyway; fixed mode is left unwaited)
            info = s.dfsph_viscosity_info()
            iters.append(info["iterations"])
    stages = {k: round(v[0] / steps, 4) for k, v in s.stage_ms().items()}
    if visc is not None and info is None:
        info = s.dfsph_viscosity_info()
    s.close()
    return stages, iters, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--spin-up", type=int, default=3)
    ap.add_argument("--lo", type=int, default=2)
    ap.add_argument("--hi", type=int, default=10)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--nu", type=float, default=1.0)
    args = ap.parse_args()
    p = default_params(capi.IISPH, False)
    sc = scene.dam_break(args.config, h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    span = args.hi - args.lo
    off, _, _ = run(sc, p, args.steps, args.spin_up, args.lo, None)
    more, _, _ = run(sc, p, args.steps, args.spin_up, args.hi, None)
    lo, _, _ = run(sc, p, args.steps, args.spin_up, args.lo, (args.nu, 0.0, 0.0, args.lo, 0))
    hi, _, _ = run(sc, p, args.steps, args.spin_up, args.lo, (args.nu, 0.0, 0.0, args.hi, 0))
    out = {"config": args.config, "n": len(sc["pos"]), "steps": args.steps, "spin_up": args.spin_up, "lo": args.lo, "hi": args.hi, "nu": args.nu,
           "ms_per_cg_iteration": round((hi["p_advect"] - lo["p_advect"]) / span, 4),
           "ms_per_dfsph_pair": round((more["p_solve"] - off["p_solve"]) / span, 4),
           "launches_per_cg_iteration": LAUNCHES_PER_ITERATION,
           "p_advect_ms": {"off": off["p_advect"], "cg_lo": lo["p_advect"], "cg_hi": hi["p_advect"]},
           "p_solve_ms": {"lo": off["p_solve"], "hi": more["p_solve"]}, "to_tolerance_1e-3": []}
    for nu in (0.01, 1.0, 100.0):
        st, iters, info = run(sc, p, args.steps, args.spin_up, args.lo, (nu, 0.0, 1e-3, 1, 0))
        out["to_tolerance_1e-3"].append({"nu": nu, "mean_iterations": float(np.mean(iters)), "max_iterations": int(np.max(iters)),
                                         "relative_residual": info["residual"] / info["rhs_norm"], "p_advect_ms": st["p_advect"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
