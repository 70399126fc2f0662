"""DFSPH against PBF and IISPH at config C3 (160^3 = 4,096,000 particles, fp32, Muller, IISPH constructor parameters, dam break with
the boundary box): per run a short untimed spin-up, then `--steps` steps timed with device events.  Each round runs DFSPH with warm
start on and off at eta = 1e-3 and at eta = 1e-4 (both loops, default minimum iterations), PBF at eta = 0.01 and IISPH.  Prints one
JSON line: ms/step, the mean iterations of both DFSPH loops, the per-stage device time (nrs_stage_ms, ms per step) and the final
averages of every run.

    python tools/bench_dfsph.py [--steps 20] [--spin-up 5] [--rounds 2] [--config C3]
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

NAMES = {capi.IISPH: "iisph", capi.PBF: "pbf", capi.DFSPH: "dfsph"}


def run(solver, sc, p, steps, spin_up, eta=None, warm=True):
    stream = torch.cuda.current_stream()
    s = capi.Solver(p, len(sc["pos"]), solver=solver, device=0, stream=stream.cuda_stream)
    if solver == capi.DFSPH:
        s.dfsph_configure(eta, 2, eta, 1, warm)
    elif solver == capi.PBF:
        s.pbf_configure(eta, 2)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(spin_up):
        s.step(1)
    s.synchronize()
    s.set_profiling(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters, div_iters = [], []
    a.record(stream)
    for _ in range(steps):
        s.step(1)
        iters.append(s.last_iterations)
        if solver == capi.DFSPH:
            div_iters.append(s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS))
    b.record(stream)
    b.synchronize()
    stages = {k: round(v[0] / steps, 4) for k, v in s.stage_ms().items()}
    out = {"solver": NAMES[solver], "ms_per_step": round(a.elapsed_time(b) / steps, 4), "mean_iterations": float(np.mean(iters)),
           "stage_ms_per_step": stages}
    if solver == capi.DFSPH:
        out["mode"] = "eta %g, warm start %s" % (eta, "on" if warm else "off")
        out["mean_divergence_iterations"] = float(np.mean(div_iters))
        out["density_avg"] = s.get_stat(capi.STAT_DFSPH_DENSITY_AVG)
        out["density_max"] = s.get_stat(capi.STAT_DENSITY_ERROR)
        out["divergence_avg"] = s.get_stat(capi.STAT_DFSPH_DIVERGENCE_AVG)
    elif solver == capi.PBF:
        out["mode"] = "eta %g" % eta
        out["density_max"] = s.get_stat(capi.STAT_DENSITY_ERROR)
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--spin-up", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--config", default="C3")
    args = ap.parse_args()
    p = default_params(capi.IISPH, False)
    sc = scene.dam_break(args.config, h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    runs = []
    for _ in range(args.rounds):
        for solver, eta, warm in ((capi.DFSPH, 1e-3, True), (capi.DFSPH, 1e-3, False), (capi.DFSPH, 1e-4, True), (capi.DFSPH, 1e-4, False),
                                  (capi.PBF, 0.01, True), (capi.IISPH, None, True)):
            runs.append(run(solver, sc, p, args.steps, args.spin_up, eta, warm))
    print(json.dumps({"config": args.config, "n": len(sc["pos"]), "steps": args.steps, "spin_up": args.spin_up, "runs": runs}))


if __name__ == "__main__":
    main()
