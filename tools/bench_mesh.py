#!/usr/bin/env python3
"""Time the mesh field (DESIGN.md "Mesh sampling"): nrs_mesh_field of an icosphere subdivided --subdiv times (5: 20480 triangles)
against a --dims^3 lattice (96: 884736 nodes) that covers it with a margin, host wall time around whole calls (they wait):
  all_ms        all four outputs: the kernel with both halves, the upload of the triangles, four copies back
  winding_ms    the winding number alone (no closest point is evaluated)
  distance_ms   the squared distance alone (no atan2 is evaluated)
and pairs_per_s = nodes * triangles / time for each.  Medians over --calls calls after --warmup, the three alternating.  One JSON
line; run five processes for a median and a spread.

The measured alternative, a workgroup staging tiles of triangles in LDS (NRS_MESH_LDS_TILE in nrs_kernels_mesh.h), is built with
  UNIT=nrs_mesh tools/build_variant.sh meshlds -DNRS_MESH_LDS_TILE=128
and selected with NEREUS_HIP_LIB=tools/_bin/libnereus_hip_meshlds.so.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nereus_amd import capi  # noqa: E402
from tests import mesh_model as mm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=5)
    ap.add_argument("--dims", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_mesh needs a GPU")
    v, t = mm.icosphere(args.subdiv, 1.0, (0.01, 0.02, 0.03))
    spacing = 2.6 / args.dims
    origin = (-1.3 + 0.37 * spacing,) * 3
    dims = (args.dims,) * 3
    pairs = float(args.dims) ** 3 * len(t)
    off = dict(winding=False, dist2=False, nearest=False, closest=False)
    calls = {
        "all_ms": lambda: capi.mesh_field(v, t, origin, spacing, dims),
        "winding_ms": lambda: capi.mesh_field(v, t, origin, spacing, dims, **dict(off, winding=True)),
        "distance_ms": lambda: capi.mesh_field(v, t, origin, spacing, dims, **dict(off, dist2=True)),
    }
    out = None
    for _ in range(args.warmup):
        for c in calls.values():
            r = c()
            out = r if "winding" in r else out
    ms = {k: [] for k in calls}
    for _ in range(args.calls):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    res = {"lib": os.path.basename(capi.LIB_PATH), "triangles": len(t), "nodes": args.dims ** 3, "pairs": pairs}
    for k, vals in ms.items():
        med = float(np.median(vals))
        res[k] = med
        res[k.replace("_ms", "_pairs_per_s")] = pairs / (1e-3 * med)
        res[k.replace("_ms", "_min_max_ms")] = [float(min(vals)), float(max(vals))]
    if out is not None and "winding" in out:
        res["inside_nodes"] = int((out["winding"] > 0.5).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
