#!/usr/bin/env python3
"""Time one step of the diffuse particles (DESIGN.md "Diffuse particles") against the SESPH step of the same state.

Scene: the dam break of config C2 (100^3 particles) after --steps steps of spin-up, a diffuse capacity of --capacity (1 M).  The context
runs on a stream of this script's, so HIP events on that stream bracket whole calls on the device's time line:
  diffuse_build_ms   nrs_diffuse_step right after an nrs_step: the sampler's grid build (hash, sort, reorder) and the six launches
  diffuse_ms         a second nrs_diffuse_step on the same state: the six launches alone
  empty_ms           the same with both rates at 0 and an empty set: what sizing the launches over the set by the capacity costs;
  empty_small_ms     ... and with a capacity of 256 instead
and step_wall_ms / diffuse_wall_ms are the host's time per nrs_step(1) / nrs_diffuse_step with nrs_synchronize on both sides.  Medians
over --calls rounds after --warmup.  One JSON line; run five processes for a median and a spread.  The per-launch times come from a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_diffuse.py).
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

SETTINGS = dict(seed=2012, tau_ta=(0.1, 0.5), tau_wc=(0.1, 1.0), tau_k=(5e-4, 4e-3), k_ta=200.0, k_wc=200.0, lifetime=(0.5, 2.0),
                k_buoyancy=2.0, k_drag=0.8, spray_below=6, bubble_above=20, max_per_particle=3)


def load_hip():
    for name in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"), "libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise SystemExit("bench_diffuse needs the HIP runtime library")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    hip = load_hip()

    def chk(rc, what):
        if rc != 0:
            raise SystemExit("bench_diffuse: %s failed with HIP error %d" % (what, rc))

    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_diffuse needs a GPU")
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    s = capi.Solver(p, n, solver=capi.SESPH, stream=stream.value)
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
        """ms between two events on the context's stream around one call"""
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

    out = {"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps, "capacity": args.capacity}
    s.diffuse_configure(capacity=args.capacity, **SETTINGS)
    step_wall, build_ms, cached_ms, diffuse_wall = [], [], [], []
    for k in range(args.warmup + args.calls):
        a = wall(lambda: s.step(1))
        b = on_device(s.diffuse_step)
        c = on_device(s.diffuse_step)
        d = wall(s.diffuse_step)
        if k >= args.warmup:
            step_wall.append(a), build_ms.append(b), cached_ms.append(c), diffuse_wall.append(d)
    alive, by_kind, dropped = s.diffuse_count()
    out.update(step_wall_ms=float(np.median(step_wall)), diffuse_build_ms=float(np.median(build_ms)), diffuse_ms=float(np.median(cached_ms)),
               diffuse_wall_ms=float(np.median(diffuse_wall)), alive=alive, by_kind=by_kind, dropped=dropped)
    out["diffuse_over_step"] = out["diffuse_build_ms"] / out["step_wall_ms"]
    quiet = dict(SETTINGS, k_ta=0.0, k_wc=0.0)
    for name, cap in (("empty_ms", args.capacity), ("empty_small_ms", 256)):
        s.diffuse_release()
        s.diffuse_configure(capacity=cap, **quiet)
        ms = [on_device(s.diffuse_step) for _ in range(args.warmup + args.calls)][args.warmup:]
        assert s.diffuse_count()[0] == 0
        out[name] = float(np.median(ms))
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
