#!/usr/bin/env python3
"""Time the field sampler's lattice entry point (DESIGN.md "Field sampling").

Scene: the dam break of config C2 (100^3 particles) after --steps steps.  Lattice: the fluid's bounding box inflated by 2h at spacing
h / 2, fields DENSITY | GRADIENT, results left on the device.  After --warmup calls (the sampler's grid is cached from the first)
--calls calls are timed with nrs_synchronize on both sides; the grid build is timed as the first call after one more step minus a cached
call.  One JSON line.  The library is the one NEREUS_HIP_LIB names (an A/B of two lattice kernels: tools/build_variant.sh, five processes
per variant, alternating).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nereus_amd import capi, scene  # noqa: E402
from nereus_amd.params import default_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--fields", type=int, default=capi.FIELD_DENSITY | capi.FIELD_GRADIENT)
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    s = capi.Solver(p, n, solver=capi.SESPH)
    if s.lib.nrs_device_count() <= 0:
        raise SystemExit("bench_sample needs a GPU")
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    P = s.params
    P["timestep"][0] = args.dt
    s.set_params(P)
    s.step(args.steps)
    pos, _ = s.download()
    lo = pos[:, :3].astype(np.float64).min(0) - 2 * h
    hi = pos[:, :3].astype(np.float64).max(0) + 2 * h
    dims = tuple(int(v) for v in np.floor((hi - lo) / (h / 2)).astype(np.int64) + 1)
    nodes = dims[0] * dims[1] * dims[2]

    def call():
        s.sample_lattice(lo, h / 2, dims, args.fields)

    def timed(k):
        s.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            call()
        s.synchronize()
        return (time.perf_counter() - t) / k

    for _ in range(args.warmup):
        call()
    per_call = timed(args.calls)
    builds = s.sample_builds()
    s.step(1)
    with_build = timed(1)
    cached = timed(1)
    assert s.sample_builds() == builds + 1
    count_nonzero = int((s.sample_result(capi.FIELD_DENSITY) != 0).sum())
    print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps, "dims": dims, "nodes": nodes,
                      "nonzero_nodes": count_nonzero, "ms_per_call": 1e3 * per_call, "nodes_per_s": nodes / per_call,
                      "grid_build_ms": 1e3 * (with_build - cached)}))


if __name__ == "__main__":
    main()
