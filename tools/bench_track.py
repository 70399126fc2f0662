#!/usr/bin/env python3
"""Time particle tracking (DESIGN.md "Particle identity and attributes") against the SESPH step of the same state.

Scene: the dam break of --config (C2: 100^3 particles) after --steps steps of spin-up.  The context runs on a stream of this script's, so
HIP events on that stream bracket whole calls on the device's time line:
  step_off_ms     nrs_step(1) with tracking off: what the parent of this feature launches
  step_ids_ms     nrs_step(1) after nrs_track_enable(0): the gather of id and birth behind the reorder
  step_attr_ms    nrs_step(1) after nrs_track_enable(NRS_TRACK_ATTR): the record rides along
  locate_ms       nrs_track_locate(0, n): the fill and the one store per living slot
  diffuse_ms      nrs_track_diffuse on all four channels with the sampler's grid already built for this state (the second of two calls),
  diffuse_first_ms the first call after a step: the sampler's grid build is part of it
Medians over --calls rounds after --warmup.  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

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
    raise SystemExit("bench_track needs the HIP runtime library")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    hip = load_hip()

    def chk(rc, what):
        if rc != 0:
            raise SystemExit("bench_track: %s failed with HIP error %d" % (what, rc))

    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    rounds = args.warmup + args.calls
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_track needs a GPU")
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
        """ms between two events on the context's stream around one call; the stream is drained first"""
        s.synchronize()
        chk(hip.hipEventRecord(ev[0], stream), "hipEventRecord")
        call()
        chk(hip.hipEventRecord(ev[1], stream), "hipEventRecord")
        chk(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = C.c_float(0)
        chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        return float(ms.value)

    def med(xs):
        return float(np.median(xs[args.warmup:]))

    def steps():
        return med([on_device(lambda: s.step(1)) for _ in range(rounds)])

    out = {"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps}
    out["step_off_ms"] = steps()
    s.track_enable(0)
    out["step_ids_ms"] = steps()
    s.track_enable(capi.TRACK_ATTR)
    out["step_attr_ms"] = steps()
    s.track_disable()
    out["step_off_again_ms"] = steps()  # (the drift of the scene over the run: the yardstick of the two differences)
    s.track_enable(capi.TRACK_ATTR)
    out["locate_ms"] = med([on_device(lambda: s._chk(s.lib.nrs_track_locate(s.h, 0, n))) for _ in range(rounds)])
    pos = s.download()[0]
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = pos[:, 0], pos[:, 1] > np.median(pos[:, 1]), pos[:, 2], 1.0
    s.track_upload(capi.TRACK_ATTRIBUTE, rec)
    kappa = (1e-4, 1e-4, 1e-4, 1e-4)
    first, again = [], []
    for _ in range(rounds):
        s.step(1)
        first.append(on_device(lambda: s.track_diffuse(kappa)))
        again.append(on_device(lambda: s.track_diffuse(kappa)))
    out.update(diffuse_first_ms=med(first), diffuse_ms=med(again))
    out["ids_over_off"] = out["step_ids_ms"] / out["step_off_ms"]
    out["attr_over_off"] = out["step_attr_ms"] / out["step_off_ms"]
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
