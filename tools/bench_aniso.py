#!/usr/bin/env python3
"""Time the anisotropic surface reconstruction (DESIGN.md "Anisotropic kernels") against the density extract it replaces.

Scene and lattice are tools/bench_surface.py's: the dam break of config C2 (100^3 particles) after --steps steps, the fluid's bounding
box inflated by 2h at spacing h / 2 (both extracts run on that one lattice; the surface phi = 0.5 lies well inside it), flags GRADIENT.
The context runs on a stream of this script's, so HIP events on that stream bracket whole calls on the device's time line:
  density_extract_ms   nrs_surface_extract at iso 0.5 restDensity: the yardstick
  sample_ms            nrs_sample_lattice with the fields that extract samples (the 27-cell gather)
  pass_a_ms            nrs_aniso_build: one record per particle (the sampler's grid is cached)
  aniso_extract_ms     nrs_surface_extract_aniso at --iso (0.5): pass A, pass B, the mesher
  pass_b_ms            the 125-cell lattice launch alone: an aniso extract at an iso no node reaches (the mesher then runs its count and scan
                       and stops) minus pass A minus the same count and scan measured on the density path (an extract at such an iso
                       minus the sampling launch)
Medians over --calls calls after --warmup, the calls alternating.  With --mesh-stats (slow on the host: not timed) the connected
components of both meshes.  One JSON line; run five processes for a median and a spread.
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
    raise SystemExit("bench_aniso needs the HIP runtime library")


def components(tri, nverts):
    """connected components of a mesh (scipy where there is one, label propagation in numpy otherwise)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    if not len(tri):
        return 0
    a, b = np.concatenate([tri[:, 0], tri[:, 1]]), np.concatenate([tri[:, 1], tri[:, 2]])
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        return int(connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(nverts, nverts)), directed=False)[0])
    except ImportError:
        parent = np.arange(nverts)
        while True:
            pa, pb = parent[a], parent[b]
            lo = np.minimum(pa, pb)
            before = parent.copy()
            np.minimum.at(parent, pa, lo)
            np.minimum.at(parent, pb, lo)
            parent = parent[parent]
            if np.array_equal(parent, before):
                return len(np.unique(parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dt", type=float, default=2.5e-4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--flags", type=int, default=capi.SURFACE_GRADIENT)
    ap.add_argument("--support", type=float, default=1.0, help="in units of h")
    ap.add_argument("--iso", type=float, default=0.5, help="of the colour field")
    ap.add_argument("--mesh-stats", action="store_true")
    args = ap.parse_args()
    lattice = args.config if not args.config[0].isdigit() else tuple(int(v) for v in args.config.split(","))
    hip = load_hip()

    def chk(rc, what):
        if rc != 0:
            raise SystemExit("bench_aniso: %s failed with HIP error %d" % (what, rc))

    p = default_params(0, False)
    h = float(p["interactionRadius"][0])
    sc = scene.dam_break(lattice, h=h, kpoly=float(p["kpoly"][0]), real=np.float32)
    n = len(sc["pos"])
    if capi.load_library().nrs_device_count() <= 0:
        raise SystemExit("bench_aniso needs a GPU")
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
    iso_d = 0.5 * float(p["restDensity"][0])
    cfg = dict(support=args.support * h)
    fields = capi.FIELD_DENSITY | (capi.FIELD_GRADIENT if args.flags & capi.SURFACE_GRADIENT else 0) | \
        (capi.FIELD_VELOCITY if args.flags & capi.SURFACE_VELOCITY else 0)
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

    out = {}
    calls = {
        "sample_ms": lambda: s.sample_lattice(lo, h / 2, dims, fields),
        "density_extract_ms": lambda: out.__setitem__("density", s.surface_extract(lo, h / 2, dims, iso_d, args.flags)),
        "density_empty_ms": lambda: s.surface_extract(lo, h / 2, dims, 1e30, args.flags),
        "pass_a_ms": lambda: s.aniso_build(cfg),
        "aniso_extract_ms": lambda: out.__setitem__("aniso", s.surface_extract_aniso(lo, h / 2, dims, args.iso, args.flags, cfg)),
        "aniso_empty_ms": lambda: s.surface_extract_aniso(lo, h / 2, dims, 1e30, args.flags, cfg),
    }
    for _ in range(args.warmup):
        for c in calls.values():
            c()
    s.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.calls):  # alternating, so that all see the same machine
        for k, c in calls.items():
            ms[k].append(on_device(c))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    med["pass_b_ms"] = med["aniso_empty_ms"] - med["pass_a_ms"] - (med["density_empty_ms"] - med["sample_ms"])
    (Vd, Td), (Va, Ta) = out["density"], out["aniso"]
    res = {"lib": os.path.basename(capi.LIB_PATH), "particles": n, "steps": args.steps, "dims": dims, "nodes": nodes, "flags": args.flags,
           "support_h": args.support, "iso": args.iso, "density_vertices": Vd, "density_triangles": Td, "aniso_vertices": Va, "aniso_triangles": Ta,
           "density_vertices_per_node": Vd / nodes, "aniso_vertices_per_node": Va / nodes,
           "pass_b_over_sample": med["pass_b_ms"] / med["sample_ms"], "aniso_over_density_extract": med["aniso_extract_ms"] / med["density_extract_ms"]}
    res.update(med)
    if args.mesh_stats:
        s.surface_extract(lo, h / 2, dims, iso_d, 0)
        res["density_components"] = components(s.surface_result(capi.MESH_TRIANGLES), Vd)
        s.surface_extract_aniso(lo, h / 2, dims, args.iso, 0, cfg)
        res["aniso_components"] = components(s.surface_result(capi.MESH_TRIANGLES), Va)
        cnt = s.aniso_result(capi.ANISO_COUNT)
        res["neighbours_mean"], res["neighbours_max"] = float(cnt.mean()), int(cnt.max())
    print(json.dumps(res))
    s.close()


if __name__ == "__main__":
    main()
