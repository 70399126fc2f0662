#!/usr/bin/env python3
"""Time the sources and sinks (DESIGN.md "Sources and sinks") against the SESPH step of the same state.

Scene: the dam break of --config (C2: 100^3 particles) after --steps steps of spin-up, with room for the emitted particles.  The context
runs on a stream of this script's, so HIP events on that stream bracket whole calls on the device's time line:
  step_ms            nrs_step(1) on a context without sinks: a coherent re-sort step
  cull_noop_ms       nrs_cull with a box that catches nothing: count, scan and the read-back of the survivor count
  step_sinks_ms      nrs_step(1) with that sink configured: the step with the no-op cull at its top
  cull_1pct_ms       nrs_cull with a box over the 1 % of the particles with the largest x: count, scan, read-back, compaction
  step_after_ms      the nrs_step(1) right after it: hash and sort in full
  layer_ms           nrs_emit_block of a --layer x --layer x 1 lattice above the fluid: one emitted layer (layer_wall_ms: the host's time
                     for it with a synchronisation on both sides, every other round)
  step_after_emit_ms the nrs_step(1) right after it
and roundtrip_wall_ms is the host's time for the same 1 % removal done by nrs_download, a numpy filter and nrs_upload_particles
(cull_1pct_wall_ms: nrs_cull timed the same way).  Medians over --calls rounds after --warmup.  One JSON line.  The per-launch times
come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_inflow.py).
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

FAR = [50.0, 50.0, 50.0, 51.0, 51.0, 51.0]


def load_hip():
    for name in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"), "libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise SystemExit("bench_inflow needs the HIP runtime library")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--layer", type=int, default=100)
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    hip = load_hip()

    def chk(rc, what):
        if rc != 0:
            raise SystemExit("bench_inflow: %s failed with HIP error %d" % (what, rc))

    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    rounds = args.warmup + args.calls
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_inflow needs a GPU")
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    s = capi.Solver(p, n + rounds * args.layer * args.layer, solver=capi.SESPH, stream=stream.value)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    P = s.params
    P["timestep"][0] = args.dt
    s.set_params(P)
    s.step(args.steps)
    s.synchronize()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        chk(hip.hipEventCreate(C.byref(e)), "hipEventCreate")

    def on_device(call):
        """ms between two events on the context's stream around one call; the stream is drained first, so that the first event does not
        take its time from work that was still queued"""
        s.synchronize()
        chk(hip.hipEventRecord(ev[0], stream), "hipEventRecord")
        call()
        chk(hip.hipEventRecord(ev[1], stream), "hipEventRecord")
        chk(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = C.c_float(0)
        chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        return float(ms.value)

    def wall(call):
        s.synchronize()
        t = time.perf_counter()
        call()
        s.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def med(xs):
        return float(np.median(xs[args.warmup:]))

    out = {"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps}
    out["step_ms"] = med([on_device(lambda: s.step(1)) for _ in range(rounds)])
    s.sinks_set([FAR], domain=True)
    out["cull_noop_ms"] = med([on_device(s.cull) for _ in range(rounds)])
    out["step_sinks_ms"] = med([on_device(lambda: s.step(1)) for _ in range(rounds)])
    out["cull_noop_over_step"] = out["cull_noop_ms"] / out["step_ms"]

    def top_percent_box(pos):
        return [float(np.percentile(pos[:, 0], 99.0)), -50.0, -50.0, 50.0, 50.0, 50.0]

    cull_ms, after_ms, removed = [], [], []
    for _ in range(rounds):
        s.sinks_set([top_percent_box(s.download()[0])])
        n0 = s.n
        cull_ms.append(on_device(s.cull))
        removed.append((n0 - s.n) / n0)
        s.sinks_set(None)
        after_ms.append(on_device(lambda: s.step(1)))
        s.step(3)  # (back to coherent re-sort steps)
    out.update(cull_1pct_ms=med(cull_ms), step_after_ms=med(after_ms), removed_fraction=float(np.median(removed)))
    walls = []
    for _ in range(rounds):
        s.sinks_set([top_percent_box(s.download()[0])])
        walls.append(wall(s.cull))
        s.sinks_set(None)
        s.step(2)
    out["cull_1pct_wall_ms"] = med(walls)

    def roundtrip():
        pos, vel = s.download()
        keep = pos[:, 0] < np.percentile(pos[:, 0], 99.0)
        s.set_particles(pos[keep], vel[keep])
    walls = []
    for _ in range(rounds):
        walls.append(wall(roundtrip))
        s.step(2)
    out["roundtrip_wall_ms"] = med(walls)
    out["particles_after_removals"] = s.n
    top = float(s.download()[0][:, 1].max()) + 2.0 * h
    layer_ms, layer_wall, after_ms = [], [], []
    for k in range(rounds):
        emit = lambda: s.emit_block((0.1, top + k * 0.8 * h, 0.1), 0.8 * h, (args.layer, 1, args.layer))  # noqa: E731
        if k % 2:
            layer_wall.append(wall(emit))
        else:
            layer_ms.append(on_device(emit))
        after_ms.append(on_device(lambda: s.step(1)))
        s.step(3)
    half = args.warmup // 2
    out.update(layer_sites=args.layer * args.layer, layer_ms=float(np.median(layer_ms[half:])), layer_wall_ms=float(np.median(layer_wall[half:])),
               step_after_emit_ms=med(after_ms), particles_end=s.n)
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
