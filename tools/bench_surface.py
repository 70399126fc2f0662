#!/usr/bin/env python3
"""Time the surface extraction (DESIGN.md "Surface extraction") against the sampling launch it starts with.

Scene and lattice are tools/bench_sample.py's: the dam break of config C2 (100^3 particles) after --steps steps, the fluid's bounding box
inflated by 2h at spacing h / 2, iso = 0.5 restDensity.  The context runs on a stream of this script's, so HIP events on that stream
bracket whole calls on the device's time line:
  sample_ms    nrs_sample_lattice with the fields the extract samples (DENSITY | GRADIENT by default): the yardstick
  extract_ms   nrs_surface_extract: that sampling launch, count + scan, the wait for the totals, the two emit launches
  mesher_ms    extract_ms - sample_ms: the mesher's four launches and the idle gap of the one wait between them
and extract_wall_ms is the host's time per extract with nrs_synchronize on both sides.  Medians over --calls calls after --warmup (the
sampler's grid is cached from the first).  algorithmic bytes per node: what the mesher must read and write once per node, see DESIGN.md.
One JSON line; run five processes for a median and a spread.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nereus_amd import capi, scene  # noqa: E402
from nereus_amd.params import default_params  # noqa: E402


def load_hip():
    for name in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"), "libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise SystemExit("bench_surface needs the HIP runtime library")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--flags", type=int, default=capi.SURFACE_GRADIENT)
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    hip = load_hip()

    def chk(rc, what):
        if rc != 0:
            raise SystemExit("bench_surface: %s failed with HIP error %d" % (what, rc))

    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_surface needs a GPU")
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    s = capi.Solver(p, n, solver=capi.SESPH, stream=stream.value)
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
    iso = 0.5 * float(p["restDensity"][0])
    fields = capi.FIELD_DENSITY | (capi.FIELD_GRADIENT if args.flags & capi.SURFACE_GRADIENT else 0) | \
        (capi.FIELD_VELOCITY if args.flags & capi.SURFACE_VELOCITY else 0) | (capi.FIELD_WALLS if args.flags & capi.SURFACE_WALLS else 0)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        chk(hip.hipEventCreate(C.byref(e)), "hipEventCreate")

    def on_device(call):
        """ms between two events on the context's stream around one call"""
        chk(hip.hipEventRecord(ev[0], stream), "hipEventRecord")
        call()
        chk(hip.hipEventRecord(ev[1], stream), "hipEventRecord")
        chk(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = C.c_float(0)
        chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        return float(ms.value)

    def sample():
        s.sample_lattice(lo, h / 2, dims, fields)

    vt = []

    def extract():
        vt.append(s.surface_extract(lo, h / 2, dims, iso, args.flags))

    for _ in range(args.warmup):
        sample()
        extract()
    s.synchronize()
    sample_ms, extract_ms, wall_ms = [], [], []
    for _ in range(args.calls):  # alternating, so that both see the same machine
        sample_ms.append(on_device(sample))
        extract_ms.append(on_device(extract))
        s.synchronize()
        t = time.perf_counter()
        extract()
        s.synchronize()
        wall_ms.append(1e3 * (time.perf_counter() - t))
    V, T = vt[-1]
    assert all(x == (V, T) for x in vt)
    real = 4
    vec4 = 4 * real
    attrs = bin(args.flags & (capi.SURFACE_GRADIENT | capi.SURFACE_VELOCITY)).count("1")
    # per node, once: the density read by the three lattice kernels, the offset and mask written and read, 8 bytes of totals per 256
    # nodes; per vertex the record and its attributes (two reads, one write each); per triangle 12 bytes
    alg_bytes = nodes * (3 * real + 2 * 4 + 2 * 1 + 8.0 / 256) + V * (vec4 + attrs * 3 * vec4) + T * 12
    sm_, em_ = float(np.median(sample_ms)), float(np.median(extract_ms))
    print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps, "dims": dims, "nodes": nodes, "flags": args.flags,
                      "vertices": V, "triangles": T, "sample_ms": sm_, "extract_ms": em_, "mesher_ms": em_ - sm_,
                      "mesher_over_sample": (em_ - sm_) / sm_, "extract_wall_ms": float(np.median(wall_ms)),
                      "mesher_algorithmic_bytes": alg_bytes, "mesher_bytes_per_node": alg_bytes / nodes,
                      "mesher_GBps": alg_bytes / (1e6 * (em_ - sm_))}))
    s.close()


if __name__ == "__main__":
    main()
