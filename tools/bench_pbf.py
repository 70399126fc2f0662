"""PBF against IISPH and PCISPH at config C3 (160^3 = 4,096,000 particles, fp32, Muller, IISPH constructor parameters, dam break with
the boundary box): per run a short untimed spin-up, then `--steps` steps timed with device events.  Each round runs PBF with a fixed
4 iterations (max_density_error 0), PBF with eta = 0.01, IISPH, PCISPH, and PBF with eta = 0.01 plus the tensile correction (k = 1e-4,
dq = 0.2), plus vorticity confinement (eps_v = 0.01), and plus both.  Prints one JSON line: ms/step, mean solver iterations, the
per-stage device time (nrs_stage_ms, ms per step) and the final max density error of every run.

    python tools/bench_pbf.py [--steps 20] [--spin-up 5] [--rounds 2] [--config C3]
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

NAMES = {capi.IISPH: "iisph", capi.PCISPH: "pcisph", capi.PBF: "pbf"}


TENSILE, VORTICITY = (1e-4, 0.2), 0.01


def run(solver, sc, p, steps, spin_up, eta=None, extras=""):
    stream = torch.cuda.current_stream()
    s = capi.Solver(p, len(sc["pos"]), solver=solver, device=0, stream=stream.cuda_stream)
    if eta is not None:
        s.pbf_configure(eta, 4 if eta == 0 else 2)
    if "s" in extras:
        s.pbf_set_tensile(*TENSILE)
    if "v" in extras:
        s.pbf_set_vorticity(VORTICITY)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(spin_up):
        s.step(1)
    s.synchronize()
    s.set_profiling(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = []
    a.record(stream)
    for _ in range(steps):
        s.step(1)
        iters.append(s.last_iterations)
    b.record(stream)
    b.synchronize()
    stages = {k: round(v[0] / steps, 4) for k, v in s.stage_ms().items()}
    out = {"solver": NAMES[solver], "ms_per_step": round(a.elapsed_time(b) / steps, 4), "mean_iterations": float(np.mean(iters)),
           "stage_ms_per_step": stages}
    if solver == capi.PBF:
        out["mode"] = ("fixed 4" if eta == 0 else "eta %g" % eta) + {"": "", "s": " +s_corr", "v": " +confinement", "sv": " +both"}[extras]
        out["density_error"] = s.get_stat(capi.STAT_DENSITY_ERROR)
        out["eps"] = s.get_stat(capi.STAT_PBF_EPSILON)
    elif solver == capi.PCISPH:
        out["density_error"] = s.get_stat(capi.STAT_DENSITY_ERROR)
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
        for solver, eta, extras in ((capi.PBF, 0.0, ""), (capi.PBF, 0.01, ""), (capi.IISPH, None, ""), (capi.PCISPH, None, ""),
                                    (capi.PBF, 0.01, "s"), (capi.PBF, 0.01, "v"), (capi.PBF, 0.01, "sv")):
            runs.append(run(solver, sc, p, args.steps, args.spin_up, eta, extras))
    print(json.dumps({"config": args.config, "n": len(sc["pos"]), "steps": args.steps, "spin_up": args.spin_up, "runs": runs}))


if __name__ == "__main__":
    main()
