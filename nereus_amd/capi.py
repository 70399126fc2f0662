"""ctypes binding of libnereus_hip.so (include/nereus_hip.h).

This is plumbing for tests/bench (Python side); the product host layer is the C++ mirror of the
reference's classes in nereus_amd/host/.  There is NO CPU fallback: if the shared library is missing
or no HIP device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

from .params import params_dtype

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NEREUS_HIP_LIB") or os.path.join(_HERE, "libnereus_hip.so")  # (override: kernel A/B builds in tools/)

SESPH, IISPH, PCISPH, PBF, DFSPH = 0, 1, 2, 3, 4
MONAGHAN, MULLER = 0, 1
FLAG_REFERENCE_ORDER = 1
FLAG_NO_FUSION = 4
FLAG_NO_SHARED_LISTS = 8
FLAG_FULL_SORT = 16
FLAG_FAST_ARITH = 32
FLAG_IISPH_SELF_BY_SLOT = 64
FLAG_NO_WALL_WORKGROUPS = 128
FLAG_STAGED_SCAN = 256
MAX_BODIES = 16
E_NOTREADY = -6
STAT_MOVERS, STAT_HIT_OVERFLOW, STAT_HIT_MEAN, STAT_HIT_MAX, STAT_UNSTAGED = 0, 1, 2, 3, 4
STAT_DENSITY_ERROR, STAT_PCISPH_DELTA, STAT_PBF_EPSILON = 5, 6, 7
STAT_DFSPH_DENSITY_AVG, STAT_DFSPH_DIVERGENCE_AVG, STAT_DFSPH_DIVERGENCE_ITERATIONS = 8, 9, 10
STAT_SLAB_PARTITION = 11   # kind of the last slab_pack: 0 compacting, 1 in place, 2 in place from the force kernel's classification
# NRS_FIELD_*: the outputs of the field sampler, and the modifier that adds the wall term to the density
FIELD_DENSITY, FIELD_GRADIENT, FIELD_VELOCITY, FIELD_COUNT, FIELD_WALLS = 1, 2, 4, 8, 16
# NRS_SURFACE_*: the flags of a surface extract (per-vertex attributes, the wall term in the density); NRS_MESH_*: one of its results
SURFACE_GRADIENT, SURFACE_VELOCITY, SURFACE_WALLS = 1, 2, 4
MESH_VERTICES, MESH_TRIANGLES, MESH_GRADIENT, MESH_VELOCITY = 1, 2, 4, 8
# NRS_ANISO_*: one result of the anisotropic kernels (nrs_aniso_build)
ANISO_CENTER, ANISO_G, ANISO_COUNT, ANISO_INDEX = 1, 2, 4, 8
# NRS_DIFFUSE_*: one result of the diffuse particles; the kinds of NRS_DIFFUSE_KIND
DIFFUSE_POS, DIFFUSE_VEL, DIFFUSE_KIND, DIFFUSE_POTENTIALS, DIFFUSE_BIRTHS, DIFFUSE_NORMALS = 0, 1, 2, 3, 4, 5
DIFFUSE_SPRAY, DIFFUSE_FOAM, DIFFUSE_BUBBLE = 0, 1, 2
# sources and sinks: slot and box caps, NRS_EMITTER_* shapes, NRS_SINK_* flags
MAX_EMITTERS, MAX_SINK_BOXES = 16, 16
EMITTER_RECT, EMITTER_DISC = 0, 1
SINK_DOMAIN = 1
# particle identity and attributes: the flag of track_enable, the NRS_TRACK_* arrays, the id that is none
TRACK_ATTR = 1
TRACK_ID, TRACK_BIRTH, TRACK_ATTRIBUTE, TRACK_SLOT_OF = 0, 1, 2, 3
TRACK_NONE = 0xFFFFFFFF
# mesh sampling: the flags of a selection rule (NRS_MESH_INSIDE, _OUTSIDE, _SNAP)
MESH_INSIDE, MESH_OUTSIDE, MESH_SNAP = 1, 2, 4

# NRS_STAGE_*
STAGE_HASH, STAGE_SORT, STAGE_REORDER, STAGE_DENSITY, STAGE_FORCES, STAGE_INTEGRATE = 1, 2, 3, 4, 5, 6
STAGE_I_DENSITY, STAGE_I_DISPLACEMENT, STAGE_I_ADVECTION, STAGE_I_SOLVE, STAGE_I_PFORCE, STAGE_I_INTEGRATE = (
    10, 11, 12, 13, 14, 15)
STAGE_P_ADVECT, STAGE_P_SOLVE, STAGE_P_INTEGRATE = 7, 8, 9
STAGE_NAMES = {1: "hash", 2: "sort", 3: "reorder", 4: "density", 5: "forces", 6: "integrate", 7: "p_advect", 8: "p_solve",
               9: "p_integrate", 10: "i_density", 11: "i_displacement", 12: "i_advection", 13: "i_solve", 14: "i_pforce",
               15: "i_integrate"}

# NRS_ARR_*: name -> (id, kind) with kind in {"v4", "s", "u"}
ARRAYS = {
    "pos": (0, "v4"), "vel": (1, "v4"), "pressure": (2, "s"), "hash": (3, "u"), "index": (4, "u"),
    "cellStart": (5, "u"), "cellEnd": (6, "u"), "sortedPos": (7, "v4"), "sortedVel": (8, "v4"),
    "dens": (9, "s"), "pres": (10, "s"), "forces": (11, "v4"), "bhash": (12, "u"), "bindex": (13, "u"),
    "bCellStart": (14, "u"), "bCellEnd": (15, "u"), "bSorted": (16, "v4"),
    "densAdv": (20, "s"), "densCorr": (21, "s"), "P_l": (22, "s"), "aii": (23, "s"), "velAdv": (24, "v4"),
    "forcesAdv": (25, "v4"), "forcesP": (26, "v4"), "diiFluid": (27, "v4"), "diiBoundary": (28, "v4"),
    "sumDij": (29, "v4"), "posPred": (30, "v4"), "vorticity": (31, "v4"), "dfsphAlpha": (32, "s"), "dfsphKappaV": (33, "s"),
    "normals": (34, "v4"), "b_body": (35, "u"),
}

# every symbol include/nereus_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "nrs_last_error", "nrs_version", "nrs_device_count", "nrs_create", "nrs_destroy", "nrs_set_params",
    "nrs_get_params", "nrs_upload_particles", "nrs_set_num_particles", "nrs_num_particles", "nrs_set_boundaries",
    "nrs_step", "nrs_step_partial", "nrs_synchronize", "nrs_download", "nrs_get_array", "nrs_device_ptr",
    "nrs_last_iterations", "nrs_set_max_iterations", "nrs_set_profiling", "nrs_stage_ms", "nrs_max_density",
    "nrs_max_velocity", "nrs_slab_configure", "nrs_slab_pack", "nrs_slab_unpack", "nrs_num_owned",
    "nrs_slab_message_bytes", "nrs_slab_histogram", "nrs_resort_stats", "nrs_snapshot_begin", "nrs_snapshot_wait",
    "nrs_get_stat", "nrs_boundary_volumes", "nrs_eval_smoothing", "nrs_iisph_predict", "nrs_iisph_iterate", "nrs_iisph_finish",
    "nrs_slab_last_counts", "nrs_pcisph_configure", "nrs_pbf_configure", "nrs_pbf_set_tensile",
    "nrs_pbf_set_vorticity", "nrs_dfsph_configure", "nrs_set_surface_akinci",
    "nrs_dfsph_set_viscosity", "nrs_dfsph_viscosity_info",
    "nrs_set_boundary_bodies", "nrs_set_body_velocity", "nrs_set_body_pose", "nrs_get_body_pose",
    "nrs_sample_points", "nrs_sample_lattice", "nrs_sample_result", "nrs_sample_device_ptr", "nrs_sample_release",
    "nrs_sample_builds",
    "nrs_surface_extract", "nrs_surface_result", "nrs_surface_device_ptr", "nrs_surface_release",
    "nrs_aniso_build", "nrs_aniso_result", "nrs_aniso_device_ptr", "nrs_aniso_release", "nrs_surface_extract_aniso",
    "nrs_diffuse_configure", "nrs_diffuse_step", "nrs_diffuse_count", "nrs_diffuse_result", "nrs_diffuse_device_ptr",
    "nrs_diffuse_upload", "nrs_diffuse_release",
    "nrs_emitter_set", "nrs_emitter_get", "nrs_emit_block", "nrs_sinks_set", "nrs_cull", "nrs_sinks_count",
    "nrs_track_enable", "nrs_track_disable", "nrs_track_info", "nrs_track_upload", "nrs_track_result", "nrs_track_device_ptr",
    "nrs_track_emit_value", "nrs_track_locate", "nrs_track_diffuse",
    "nrs_mesh_field", "nrs_mesh_particles", "nrs_emit_mesh",
]


class NrsAnisoConfig(C.Structure):
    _fields_ = [("support", C.c_double), ("lam", C.c_double), ("k_r", C.c_double), ("k_n", C.c_double), ("n_eps", C.c_uint32),
                ("reserved", C.c_uint32)]


class NrsEmitter(C.Structure):
    _fields_ = [
        ("shape", C.c_uint32), ("enabled", C.c_uint32), ("center", C.c_double * 3), ("direction", C.c_double * 3),
        ("half_extent", C.c_double * 2), ("speed", C.c_double), ("spacing", C.c_double), ("max_particles", C.c_uint64),
    ]


class NrsSinkConfig(C.Structure):
    _fields_ = [
        ("flags", C.c_uint32), ("nboxes", C.c_uint32), ("interval", C.c_uint32), ("reserved", C.c_uint32),
        ("boxes", (C.c_double * 6) * MAX_SINK_BOXES),
    ]


class NrsDiffuseConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("capacity", C.c_uint32), ("seed", C.c_uint64),
        ("tau_ta", C.c_double * 2), ("tau_wc", C.c_double * 2), ("tau_k", C.c_double * 2),
        ("k_ta", C.c_double), ("k_wc", C.c_double), ("lifetime", C.c_double * 2),
        ("k_buoyancy", C.c_double), ("k_drag", C.c_double),
        ("spray_below", C.c_uint32), ("bubble_above", C.c_uint32), ("max_per_particle", C.c_uint32), ("reserved", C.c_uint32),
    ]


class NrsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("solver", C.c_int32), ("precision", C.c_int32),
        ("kernel_set", C.c_int32), ("surface_tension", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
        ("capacity", C.c_uint64), ("stream", C.c_void_p),
    ]


class NrsLattice(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("dims", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class NrsMesh(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("nv", C.c_uint64), ("triangles", C.c_void_p), ("nt", C.c_uint64)]


class NrsMeshRule(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("dmin", C.c_double), ("dmax", C.c_double)]


class NereusError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """Load libnereus_hip.so (once).  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise NereusError(
            "libnereus_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nereus_amd/csrc`; there is no CPU fallback" % path)
    lib = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.nrs_last_error.restype = C.c_char_p
    lib.nrs_version.restype = C.c_uint32
    lib.nrs_device_count.restype = i32
    lib.nrs_create.argtypes = [C.POINTER(NrsConfig), vp, C.POINTER(vp)]
    lib.nrs_destroy.argtypes = [vp]
    lib.nrs_set_params.argtypes = [vp, vp]
    lib.nrs_get_params.argtypes = [vp, vp]
    lib.nrs_upload_particles.argtypes = [vp, vp, vp, vp, u64, u64]
    lib.nrs_set_num_particles.argtypes = [vp, u64]
    lib.nrs_num_particles.argtypes = [vp]
    lib.nrs_num_particles.restype = u64
    lib.nrs_set_boundaries.argtypes = [vp, vp, vp, u64, i32]
    dp = C.POINTER(C.c_double)
    lib.nrs_set_boundary_bodies.argtypes = [vp, vp, u64, C.c_uint32]
    lib.nrs_set_body_velocity.argtypes = [vp, C.c_uint32, dp, dp]
    lib.nrs_set_body_pose.argtypes = [vp, C.c_uint32, dp, dp]
    lib.nrs_get_body_pose.argtypes = [vp, C.c_uint32, dp, dp]
    lib.nrs_step.argtypes = [vp, i32]
    lib.nrs_step_partial.argtypes = [vp, i32]
    lib.nrs_synchronize.argtypes = [vp]
    lib.nrs_download.argtypes = [vp, vp, vp, vp]
    lib.nrs_get_array.argtypes = [vp, i32, vp, u64, C.POINTER(u64)]
    lib.nrs_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_last_iterations.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.nrs_set_max_iterations.argtypes = [vp, C.c_uint32]
    lib.nrs_pcisph_configure.argtypes = [vp, C.c_double, C.c_uint32, C.c_double, C.c_double]
    lib.nrs_pbf_configure.argtypes = [vp, C.c_double, C.c_uint32, C.c_double, C.c_double]
    lib.nrs_pbf_set_tensile.argtypes = [vp, C.c_double, C.c_double]
    lib.nrs_pbf_set_vorticity.argtypes = [vp, C.c_double]
    lib.nrs_dfsph_configure.argtypes = [vp, C.c_double, C.c_uint32, C.c_double, C.c_uint32, i32]
    lib.nrs_set_surface_akinci.argtypes = [vp, C.c_double, C.c_double]
    lib.nrs_dfsph_set_viscosity.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32]
    lib.nrs_dfsph_viscosity_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.nrs_set_profiling.argtypes = [vp, C.c_uint32]
    lib.nrs_stage_ms.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    lib.nrs_max_density.argtypes = [vp, C.POINTER(C.c_double)]
    lib.nrs_max_velocity.argtypes = [vp, C.POINTER(C.c_double)]
    lib.nrs_slab_configure.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    lib.nrs_slab_pack.argtypes = [vp, vp, vp, u64, C.POINTER(C.c_uint32)]
    lib.nrs_slab_unpack.argtypes = [vp, vp, vp, u64]
    lib.nrs_slab_last_counts.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.nrs_num_owned.argtypes = [vp]
    lib.nrs_num_owned.restype = u64
    lib.nrs_slab_message_bytes.argtypes = [u64, i32]
    lib.nrs_slab_message_bytes.restype = u64
    lib.nrs_slab_histogram.argtypes = [vp, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.nrs_resort_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_get_stat.argtypes = [vp, i32, C.POINTER(C.c_double)]
    lib.nrs_iisph_predict.argtypes = [vp]
    lib.nrs_iisph_iterate.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    lib.nrs_iisph_finish.argtypes = [vp]
    lib.nrs_eval_smoothing.argtypes = [i32, i32, u64, vp, vp, C.c_double, C.c_double, C.c_double, vp]
    lib.nrs_boundary_volumes.argtypes = [i32, i32, vp, u64, C.c_double, vp]
    lib.nrs_snapshot_begin.argtypes = [vp, i32]
    lib.nrs_snapshot_wait.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_sample_points.argtypes = [vp, vp, u64, C.c_uint32]
    lib.nrs_sample_lattice.argtypes = [vp, C.POINTER(NrsLattice), C.c_uint32]
    lib.nrs_sample_result.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(u64)]
    lib.nrs_sample_device_ptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_sample_release.argtypes = [vp]
    lib.nrs_sample_builds.argtypes = [vp, C.POINTER(u64)]
    lib.nrs_surface_extract.argtypes = [vp, C.POINTER(NrsLattice), C.c_double, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_surface_result.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(u64)]
    lib.nrs_surface_device_ptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_surface_release.argtypes = [vp]
    lib.nrs_aniso_build.argtypes = [vp, C.POINTER(NrsAnisoConfig)]
    lib.nrs_aniso_result.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(u64)]
    lib.nrs_aniso_device_ptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_aniso_release.argtypes = [vp]
    lib.nrs_surface_extract_aniso.argtypes = [vp, C.POINTER(NrsLattice), C.c_double, C.c_uint32, C.POINTER(NrsAnisoConfig), C.POINTER(u64),
                                              C.POINTER(u64)]
    lib.nrs_diffuse_configure.argtypes = [vp, C.POINTER(NrsDiffuseConfig)]
    lib.nrs_diffuse_step.argtypes = [vp, C.c_double]
    lib.nrs_diffuse_count.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_diffuse_result.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(u64)]
    lib.nrs_diffuse_device_ptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_diffuse_upload.argtypes = [vp, vp, vp, u64]
    lib.nrs_diffuse_release.argtypes = [vp]
    lib.nrs_emitter_set.argtypes = [vp, C.c_uint32, C.POINTER(NrsEmitter)]
    lib.nrs_emitter_get.argtypes = [vp, C.c_uint32, C.POINTER(NrsEmitter), C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_emit_block.argtypes = [vp, C.POINTER(NrsLattice), C.POINTER(C.c_double), C.POINTER(u64)]
    lib.nrs_sinks_set.argtypes = [vp, C.POINTER(NrsSinkConfig)]
    lib.nrs_cull.argtypes = [vp, C.POINTER(u64)]
    lib.nrs_sinks_count.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.nrs_track_enable.argtypes = [vp, C.c_uint32]
    lib.nrs_track_disable.argtypes = [vp]
    lib.nrs_track_info.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_uint32), C.POINTER(u64)]
    lib.nrs_track_upload.argtypes = [vp, C.c_uint32, vp, u64, u64]
    lib.nrs_track_result.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(u64)]
    lib.nrs_track_device_ptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(u64)]
    lib.nrs_track_emit_value.argtypes = [vp, C.c_int32, dp]
    lib.nrs_track_locate.argtypes = [vp, u64, u64]
    lib.nrs_track_diffuse.argtypes = [vp, dp, C.c_double]
    lib.nrs_mesh_field.argtypes = [i32, C.POINTER(NrsMesh), C.POINTER(NrsLattice), vp, vp, vp, vp]
    lib.nrs_mesh_particles.argtypes = [i32, i32, C.POINTER(NrsMesh), C.POINTER(NrsLattice), C.POINTER(NrsMeshRule), vp, u64, C.POINTER(u64)]
    lib.nrs_emit_mesh.argtypes = [vp, C.POINTER(NrsMesh), C.POINTER(NrsLattice), C.POINTER(NrsMeshRule), dp, C.POINTER(u64)]
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def boundary_volumes(bi4, h, double=False, device=-1):
    """Akinci volumes of the boundary particles bi4 (n,4) on the device (nrs_boundary_volumes); returns (n,) SReal."""
    lib = load_library()
    real = np.float64 if double else np.float32
    bi4 = np.ascontiguousarray(bi4, dtype=real).reshape(-1, 4)
    out = np.empty(bi4.shape[0], dtype=real)
    rc = lib.nrs_boundary_volumes(int(device), 64 if double else 32, _ptr(bi4), bi4.shape[0], float(h), _ptr(out))
    if rc != 0:
        raise NereusError("libnereus_hip error %d: %s" % (rc, lib.nrs_last_error().decode()))
    return out


def _lattice(origin, spacing, dims):
    L = NrsLattice()
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    for a in range(3):
        L.origin[a], L.spacing[a], L.dims[a] = float(origin[a]), float(sp[a]), int(dims[a])
    return L


def _mesh(vertices, triangles):
    """an nrs_mesh over vertices (nv, 3) double and triangles (nt, 3) uint32; returns (struct, the arrays it points into)"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    m = NrsMesh(v.ctypes.data if v.size else None, v.shape[0], t.ctypes.data if t.size else None, t.shape[0])
    return m, (v, t)


def _mesh_rule(flags, dmin, dmax, reserved=0):
    return NrsMeshRule(int(flags), int(reserved), float(dmin), float(dmax))


def mesh_field(vertices, triangles, origin, spacing, dims, winding=True, dist2=True, nearest=True, closest=True, device=-1):
    """winding number, squared distance, nearest triangle and closest point of a triangle mesh at the nodes of a lattice
    (nrs_mesh_field); returns a dict with the outputs asked for: "winding" (m,), "dist2" (m,), "nearest" (m,) uint32,
    "closest" (m, 3), m the nodes in linear index order"""
    lib = load_library()
    M, keep = _mesh(vertices, triangles)
    L = _lattice(origin, spacing, dims)
    m = int(dims[0]) * int(dims[1]) * int(dims[2])
    out = {}
    if winding:
        out["winding"] = np.empty(m, np.float64)
    if dist2:
        out["dist2"] = np.empty(m, np.float64)
    if nearest:
        out["nearest"] = np.empty(m, np.uint32)
    if closest:
        out["closest"] = np.empty((m, 3), np.float64)
    rc = lib.nrs_mesh_field(int(device), C.byref(M), C.byref(L), _ptr(out.get("winding")), _ptr(out.get("dist2")),
                            _ptr(out.get("nearest")), _ptr(out.get("closest")))
    if rc != 0:
        raise NereusError("libnereus_hip error %d: %s" % (rc, lib.nrs_last_error().decode()))
    return out


def mesh_particles(vertices, triangles, origin, spacing, dims, flags=MESH_INSIDE, dmin=0.0, dmax=float("inf"), double=False,
                   count_only=False, capacity=None, device=-1):
    """the lattice nodes a rule selects as particles (nrs_mesh_particles): (count, 4) SReal, w = 1, in linear index order; with
    MESH_SNAP the closest points on the mesh.  Two calls: the count, then the particles.  count_only: just the count.  capacity: the room offered (default: what is needed;
    less raises NereusError with NRS_E_CAPACITY)"""
    lib = load_library()
    M, keep = _mesh(vertices, triangles)
    L = _lattice(origin, spacing, dims)
    R = _mesh_rule(flags, dmin, dmax)
    real = np.float64 if double else np.float32
    count = C.c_uint64(0)
    rc = lib.nrs_mesh_particles(int(device), 64 if double else 32, C.byref(M), C.byref(L), C.byref(R), None, 0, C.byref(count))
    if rc != 0:
        raise NereusError("libnereus_hip error %d: %s" % (rc, lib.nrs_last_error().decode()))
    if count_only:
        return int(count.value)
    cap = int(count.value) if capacity is None else int(capacity)
    out = np.empty((cap, 4), real)
    rc = lib.nrs_mesh_particles(int(device), 64 if double else 32, C.byref(M), C.byref(L), C.byref(R), _ptr(out) if cap else None, cap,
                                C.byref(count))
    if rc != 0:
        raise NereusError("libnereus_hip error %d: %s" % (rc, lib.nrs_last_error().decode()))
    return out[:int(count.value)]


def eval_smoothing(which, r, s, h, c0, c1, double=False):
    """device smoothing kernel / vector helper number `which` on separations r (n,3) [and s]; returns (n,3) (nrs_eval_smoothing)"""
    lib = load_library()
    real = np.float64 if double else np.float32
    r = np.ascontiguousarray(r, dtype=real)
    s = None if s is None else np.ascontiguousarray(s, dtype=real)
    out = np.zeros_like(r)
    rc = lib.nrs_eval_smoothing(64 if double else 32, int(which), r.shape[0], _ptr(r), _ptr(s), float(h), float(c0), float(c1), _ptr(out))
    if rc != 0:
        raise NereusError("libnereus_hip error %d: %s" % (rc, lib.nrs_last_error().decode()))
    return out


class Solver:
    """Thin object wrapper over an nrs_ctx (device-resident SESPH / IISPH / PCISPH / PBF / DFSPH solver)."""

    def __init__(self, params, capacity, solver=SESPH, double=False, kernel_set=MULLER, surface_tension=True,
                 reference_order=False, device=-1, stream=None, flags=0):
        self.lib = load_library()
        self.double = bool(double)
        self.real = np.float64 if double else np.float32
        self.solver = solver
        p = np.array(params, dtype=params_dtype(double)).reshape(1).copy()
        cfg = NrsConfig()
        cfg.struct_size = C.sizeof(NrsConfig)
        cfg.device = device
        cfg.solver = solver
        cfg.precision = 64 if double else 32
        cfg.kernel_set = kernel_set
        cfg.surface_tension = int(bool(surface_tension))
        cfg.flags = (FLAG_REFERENCE_ORDER if reference_order else 0) | int(flags)
        cfg.capacity = int(capacity)
        cfg.stream = stream
        h = C.c_void_p()
        self.h = None
        self._chk(self.lib.nrs_create(C.byref(cfg), _ptr(p), C.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise NereusError("libnereus_hip error %d: %s" % (rc, self.lib.nrs_last_error().decode()))

    def close(self):
        if self.h:
            self.lib.nrs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def params(self):
        p = np.zeros(1, dtype=params_dtype(self.double))
        self._chk(self.lib.nrs_get_params(self.h, _ptr(p)))
        return p

    def set_params(self, params):
        p = np.array(params, dtype=params_dtype(self.double)).reshape(1).copy()
        self._chk(self.lib.nrs_set_params(self.h, _ptr(p)))

    def set_particles(self, pos4, vel4=None, pres=None, first=0):
        pos4 = np.ascontiguousarray(pos4, dtype=self.real).reshape(-1, 4)
        n = pos4.shape[0]
        vel4 = None if vel4 is None else np.ascontiguousarray(vel4, dtype=self.real)
        pres = None if pres is None else np.ascontiguousarray(pres, dtype=self.real)
        if first == 0:
            self._chk(self.lib.nrs_set_num_particles(self.h, 0))
        self._chk(self.lib.nrs_upload_particles(self.h, _ptr(pos4), _ptr(vel4), _ptr(pres), first, n))

    def set_boundaries(self, bi4, vbi, update_grid=True):
        if bi4 is None or len(bi4) == 0:
            self._chk(self.lib.nrs_set_boundaries(self.h, None, None, 0, 0))
            return
        bi4 = np.ascontiguousarray(bi4, dtype=self.real).reshape(-1, 4)
        vbi = np.ascontiguousarray(vbi, dtype=self.real).reshape(-1)
        assert vbi.shape[0] == bi4.shape[0]
        self._chk(self.lib.nrs_set_boundaries(self.h, _ptr(bi4), _ptr(vbi), bi4.shape[0], int(update_grid)))

    # ---- kinematic boundary bodies -----------------------------------------------------------------
    def set_boundary_bodies(self, body_of, nbodies):
        """group the boundary particles of the last set_boundaries into rigid bodies (nrs_set_boundary_bodies): body_of[i] in
        0 .. nbodies-1, body 0 the static world; None or nbodies <= 1 clears the assignment"""
        if body_of is None:
            self._chk(self.lib.nrs_set_boundary_bodies(self.h, None, 0, int(nbodies)))
            return
        body_of = np.ascontiguousarray(body_of, dtype=np.uint32).reshape(-1)
        self._chk(self.lib.nrs_set_boundary_bodies(self.h, _ptr(body_of), body_of.shape[0], int(nbodies)))

    def set_body_velocity(self, body, v, omega=(0.0, 0.0, 0.0)):
        """world-frame linear velocity of the body's origin and angular velocity about it, held until changed"""
        v, w = (C.c_double * 3)(*[float(a) for a in v]), (C.c_double * 3)(*[float(a) for a in omega])
        self._chk(self.lib.nrs_set_body_velocity(self.h, int(body), v, w))

    def set_body_pose(self, body, x, q=(1.0, 0.0, 0.0, 0.0)):
        """teleport: origin x and orientation q = (w, x, y, z), normalised by the library"""
        x, q = (C.c_double * 3)(*[float(a) for a in x]), (C.c_double * 4)(*[float(a) for a in q])
        self._chk(self.lib.nrs_set_body_pose(self.h, int(body), x, q))

    def body_pose(self, body):
        """(x, q) of the body as the last step used it, float64 arrays"""
        x, q = (C.c_double * 3)(), (C.c_double * 4)()
        self._chk(self.lib.nrs_get_body_pose(self.h, int(body), x, q))
        return np.array(x[:]), np.array(q[:])

    @property
    def n(self):
        return int(self.lib.nrs_num_particles(self.h))

    def step(self, nsteps=1):
        self._chk(self.lib.nrs_step(self.h, int(nsteps)))

    def step_partial(self, stage):
        self._chk(self.lib.nrs_step_partial(self.h, int(stage)))

    def synchronize(self):
        self._chk(self.lib.nrs_synchronize(self.h))

    def download(self, pressure=False):
        n = self.n
        pos = np.empty((n, 4), self.real)
        vel = np.empty((n, 4), self.real)
        pres = np.empty(n, self.real) if pressure else None
        self._chk(self.lib.nrs_download(self.h, _ptr(pos), _ptr(vel), _ptr(pres)))
        return (pos, vel, pres) if pressure else (pos, vel)

    def get(self, name):
        aid, kind = ARRAYS[name]
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_get_array(self.h, aid, None, 0, C.byref(nbytes)))
        dt = np.uint32 if kind == "u" else self.real
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_get_array(self.h, aid, _ptr(a), nbytes.value, None))
        return a.reshape(-1, 4) if kind == "v4" else a

    def device_ptr(self, name):
        aid, _ = ARRAYS[name]
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_device_ptr(self.h, aid, C.byref(p), C.byref(b)))
        return p.value, b.value

    @property
    def last_iterations(self):
        it = C.c_uint32(0)
        self._chk(self.lib.nrs_last_iterations(self.h, C.byref(it)))
        return it.value

    def set_max_iterations(self, m):
        self._chk(self.lib.nrs_set_max_iterations(self.h, int(m)))

    def pcisph_configure(self, max_density_error=0.01, min_iters=3, prototype_spacing=0.0, delta=0.0):
        """PCISPH loop settings (nrs_pcisph_configure): exit error, minimum iterations, prototype lattice spacing (0 = cbrt(m / rho0)),
        pressure scale delta (0 = from the prototype)"""
        self._chk(self.lib.nrs_pcisph_configure(self.h, float(max_density_error), int(min_iters), float(prototype_spacing), float(delta)))

    def pbf_configure(self, max_density_error=0.01, min_iters=2, relaxation=0.01, xsph=0.0):
        """PBF loop settings (nrs_pbf_configure): exit error (0 = exactly min_iters iterations, nothing read back), minimum iterations,
        eps = relaxation * D_proto, XSPH factor (0 = off)"""
        self._chk(self.lib.nrs_pbf_configure(self.h, float(max_density_error), int(min_iters), float(relaxation), float(xsph)))

    def pbf_set_tensile(self, k=0.0, dq=0.2):
        """PBF tensile correction (nrs_pbf_set_tensile): s_ij = -k (W(x*_ij) / W((dq h, 0, 0)))^4 on fluid pairs (k = 0 = off)"""
        self._chk(self.lib.nrs_pbf_set_tensile(self.h, float(k), float(dq)))

    def pbf_set_vorticity(self, eps_v=0.0):
        """PBF vorticity confinement (nrs_pbf_set_vorticity): vel += dt eps_v (N x omega) at the end of the step (0 = off)"""
        self._chk(self.lib.nrs_pbf_set_vorticity(self.h, float(eps_v)))

    def dfsph_configure(self, max_density_error=1e-3, min_iters=2, max_divergence_error=1e-3, min_divergence_iters=1, warm_start=True):
        """DFSPH settings (nrs_dfsph_configure): per loop the exit average error (0 = exactly the minimum, nothing read back) and the
        minimum iterations (min_divergence_iters = 0: no divergence solve), and the warm start from the previous step's K / Kv"""
        self._chk(self.lib.nrs_dfsph_configure(self.h, float(max_density_error), int(min_iters), float(max_divergence_error),
                                               int(min_divergence_iters), int(warm_start)))

    def surface_akinci(self, gamma=0.0, beta=0.0):
        """Akinci surface tension gamma and wall adhesion beta_a on a PCISPH / PBF / DFSPH context (nrs_set_surface_akinci; 0, 0 = off)"""
        self._chk(self.lib.nrs_set_surface_akinci(self.h, float(gamma), float(beta)))

    def dfsph_set_viscosity(self, nu=0.0, nu_boundary=0.0, tolerance=1e-3, min_iters=1, max_iters=0):
        """the implicit viscosity solve of the DFSPH step (nrs_dfsph_set_viscosity): (I - dt nu L) u = vel_adv by conjugate gradients
        behind the advection launch; nu = 0 = off, nu_boundary = wall friction (0 = slip), tolerance = 0 = exactly min_iters iterations
        and nothing read back, max_iters = 0 = 100"""
        self._chk(self.lib.nrs_dfsph_set_viscosity(self.h, float(nu), float(nu_boundary), float(tolerance), int(min_iters), int(max_iters)))

    def dfsph_viscosity_info(self):
        """dict(on, iterations, residual, rhs_norm) of the last step's implicit viscosity solve (nrs_dfsph_viscosity_info); waits"""
        on, it, res, rhs = C.c_int(0), C.c_uint32(0), C.c_double(0), C.c_double(0)
        self._chk(self.lib.nrs_dfsph_viscosity_info(self.h, C.byref(on), C.byref(it), C.byref(res), C.byref(rhs)))
        return dict(on=bool(on.value), iterations=it.value, residual=res.value, rhs_norm=rhs.value)

    def set_profiling(self, stages=True):
        """stages: True = all, False = off, or an iterable of stage ids."""
        if stages is True:
            mask = 0xFFFFFFFF
        elif not stages:
            mask = 0
        else:
            mask = 0
            for s in stages:
                mask |= 1 << int(s)
        self._chk(self.lib.nrs_set_profiling(self.h, mask))

    def stage_ms(self):
        """{stage name: (ms summed over the steps since the last set_profiling call, launches)}; synchronizes"""
        out = {}
        for sid, name in STAGE_NAMES.items():
            ms, cnt = C.c_float(0), C.c_uint32(0)
            self._chk(self.lib.nrs_stage_ms(self.h, sid, C.byref(ms), C.byref(cnt)))
            if cnt.value:
                out[name] = (ms.value, cnt.value)
        return out

    # ---- slab decomposition ------------------------------------------------------------------------
    def slab_configure(self, cell_lo, cell_hi, halo_cells=2):
        self._chk(self.lib.nrs_slab_configure(self.h, int(cell_lo), int(cell_hi), int(halo_cells)))

    def slab_pack(self, send_left_ptr, send_right_ptr, capacity, want_counts=True):
        """want_counts=False: do not wait for the device (the counts are read back inside slab_unpack; slab_last_counts())"""
        if not want_counts:
            self._chk(self.lib.nrs_slab_pack(self.h, send_left_ptr, send_right_ptr, int(capacity), None))
            return None
        counts = (C.c_uint32 * 6)()
        self._chk(self.lib.nrs_slab_pack(self.h, send_left_ptr, send_right_ptr, int(capacity), counts))
        return list(counts)

    def slab_last_counts(self):
        counts = (C.c_uint32 * 6)()
        self._chk(self.lib.nrs_slab_last_counts(self.h, counts))
        return list(counts)

    def slab_unpack(self, recv_left_ptr, recv_right_ptr, capacity):
        self._chk(self.lib.nrs_slab_unpack(self.h, recv_left_ptr, recv_right_ptr, int(capacity)))

    def slab_histogram(self, first_cell, ncells):
        out = (C.c_uint32 * int(ncells))()
        self._chk(self.lib.nrs_slab_histogram(self.h, int(first_cell), int(ncells), out))
        return np.frombuffer(out, dtype=np.uint32).copy()

    def snapshot_begin(self, with_vel=False):
        """start an asynchronous copy of the current positions (and velocities) to pinned host memory"""
        self._chk(self.lib.nrs_snapshot_begin(self.h, 1 if with_vel else 0))

    def snapshot_wait(self, block=True):
        """oldest pending snapshot as (pos, vel or None, step) — numpy views of the library's pinned buffers, valid until
        two more snapshot_begin calls — or None if block is False and the transfer is still running"""
        pp, pv, n, step = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = self.lib.nrs_snapshot_wait(self.h, 1 if block else 0, C.byref(pp), C.byref(pv), C.byref(n), C.byref(step))
        if rc == E_NOTREADY:
            return None
        self._chk(rc)
        ct = C.c_double if self.real == np.float64 else C.c_float

        def view(ptr):
            if not ptr.value or not n.value:
                return np.empty((0, 4), self.real) if ptr.value or not n.value else None
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(int(n.value), 4))

        return view(pp), (view(pv) if pv.value else None), int(step.value)

    def resort_stats(self):
        """(steps that used the coherent re-sort path, how many of them fell back to the full radix sort)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.nrs_resort_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def iisph_predict(self):
        self._chk(self.lib.nrs_iisph_predict(self.h))

    def iisph_iterate(self):
        """one solver iteration; returns (sum of corrected densities over the owned particles, their number)"""
        sm, cnt = C.c_double(0), C.c_uint64(0)
        self._chk(self.lib.nrs_iisph_iterate(self.h, C.byref(sm), C.byref(cnt)))
        return sm.value, int(cnt.value)

    def iisph_finish(self):
        self._chk(self.lib.nrs_iisph_finish(self.h))

    def get_stat(self, which):
        v = C.c_double()
        self._chk(self.lib.nrs_get_stat(self.h, int(which), C.byref(v)))
        return v.value

    # ---- field sampling -----------------------------------------------------------------------------
    def sample_points(self, points4, fields):
        """evaluate `fields` (FIELD_* flags) at the rows of points4 (m, 4), w ignored (nrs_sample_points); does not wait for the device"""
        pts = np.ascontiguousarray(points4, dtype=self.real).reshape(-1, 4)
        self._chk(self.lib.nrs_sample_points(self.h, _ptr(pts) if len(pts) else None, pts.shape[0], int(fields)))

    _lattice = staticmethod(_lattice)

    def sample_lattice(self, origin, spacing, dims, fields):
        """evaluate `fields` on the dims[0] x dims[1] x dims[2] nodes origin + idx * spacing (nrs_sample_lattice); spacing: a number
        or one per axis"""
        L = self._lattice(origin, spacing, dims)
        self._chk(self.lib.nrs_sample_lattice(self.h, C.byref(L), int(fields)))

    def sample_result(self, field):
        """one field of the last sample call on the host: (m,) SReal density, (m, 4) gradient / velocity, (m,) uint32 count"""
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_sample_result(self.h, int(field), None, 0, C.byref(nbytes)))
        dt = np.uint32 if field == FIELD_COUNT else self.real
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_sample_result(self.h, int(field), _ptr(a), nbytes.value, None))
        return a.reshape(-1, 4) if field in (FIELD_GRADIENT, FIELD_VELOCITY) else a

    def sample_device_ptr(self, field):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_sample_device_ptr(self.h, int(field), C.byref(p), C.byref(b)))
        return p.value, b.value

    def sample_builds(self):
        """how many times the sampler built its particle grid since the context was created (nrs_sample_builds)"""
        b = C.c_uint64(0)
        self._chk(self.lib.nrs_sample_builds(self.h, C.byref(b)))
        return int(b.value)

    def sample_release(self):
        self._chk(self.lib.nrs_sample_release(self.h))

    # ---- surface extraction ---------------------------------------------------------------------------
    def surface_extract(self, origin, spacing, dims, iso, flags=0):
        """the iso-surface rho = iso on the lattice as a triangle mesh on the device (nrs_surface_extract): samples the lattice
        (sample_result(FIELD_DENSITY) afterwards is the lattice the mesh was cut from), meshes it, waits for the totals; -> (V, T)"""
        L = self._lattice(origin, spacing, dims)
        v, t = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.nrs_surface_extract(self.h, C.byref(L), float(iso), int(flags), C.byref(v), C.byref(t)))
        return int(v.value), int(t.value)

    def surface_result(self, which):
        """one result of the last extract on the host: (V, 4) SReal vertices (x, y, z, t) / gradient / velocity, (T, 3) uint32 triangles"""
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_surface_result(self.h, int(which), None, 0, C.byref(nbytes)))
        dt = np.uint32 if which == MESH_TRIANGLES else self.real
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_surface_result(self.h, int(which), _ptr(a), nbytes.value, None))
        return a.reshape(-1, 3) if which == MESH_TRIANGLES else a.reshape(-1, 4)

    def surface_device_ptr(self, which):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_surface_device_ptr(self.h, int(which), C.byref(p), C.byref(b)))
        return p.value, b.value

    def surface_release(self):
        self._chk(self.lib.nrs_surface_release(self.h))

    # ---- anisotropic surface reconstruction ------------------------------------------------------------
    @staticmethod
    def _aniso_config(cfg):
        """None (the library's defaults) or a dict with any of support, lam, k_r, k_n, n_eps, reserved over those defaults (support 0 = h)"""
        if cfg is None:
            return None
        c = NrsAnisoConfig(0.0, 0.9, 4.0, 0.5, 25, 0)
        for k, v in cfg.items():
            if k not in ("support", "lam", "k_r", "k_n", "n_eps", "reserved"):
                raise KeyError(k)
            setattr(c, k, v)
        return C.byref(c)

    def aniso_build(self, cfg=None):
        """the anisotropic kernel of every fluid particle, in the sampler's sorted order (nrs_aniso_build); does not wait for the device"""
        self._chk(self.lib.nrs_aniso_build(self.h, self._aniso_config(cfg)))

    def aniso_result(self, which):
        """one result of the last aniso_build on the host: ANISO_CENTER (N, 4) centre + bound, ANISO_G (N, 8) G00 G01 G02 G11 G12 G22
        weight 0, ANISO_COUNT / ANISO_INDEX (N,) uint32"""
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_aniso_result(self.h, int(which), None, 0, C.byref(nbytes)))
        dt = np.uint32 if which in (ANISO_COUNT, ANISO_INDEX) else self.real
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_aniso_result(self.h, int(which), _ptr(a), nbytes.value, None))
        return a.reshape(-1, 4) if which == ANISO_CENTER else a.reshape(-1, 8) if which == ANISO_G else a

    def aniso_device_ptr(self, which):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_aniso_device_ptr(self.h, int(which), C.byref(p), C.byref(b)))
        return p.value, b.value

    def aniso_release(self):
        self._chk(self.lib.nrs_aniso_release(self.h))

    def surface_extract_aniso(self, origin, spacing, dims, iso=0.5, flags=0, cfg=None):
        """the iso-surface phi = iso of the anisotropic colour field on the lattice (nrs_surface_extract_aniso): builds the kernels, writes
        phi (and the attributes) into the sampler's result arrays, meshes them, waits for the totals; -> (V, T); the mesh comes back through
        surface_result"""
        L = self._lattice(origin, spacing, dims)
        v, t = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.nrs_surface_extract_aniso(self.h, C.byref(L), float(iso), int(flags), self._aniso_config(cfg), C.byref(v), C.byref(t)))
        return int(v.value), int(t.value)

    # ---- diffuse particles ----------------------------------------------------------------------------
    def diffuse_configure(self, capacity, seed=0, tau_ta=(5.0, 20.0), tau_wc=(2.0, 8.0), tau_k=(5.0, 50.0), k_ta=4000.0, k_wc=50000.0,
                          lifetime=(2.0, 5.0), k_buoyancy=2.0, k_drag=0.8, spray_below=6, bubble_above=20, max_per_particle=8,
                          struct_size=None, reserved=0):
        """configure the context's diffuse particles (nrs_diffuse_configure): spray, foam and bubbles after Ihmsen et al. 2012; allocates
        nothing, restarts the step counter and `dropped`, keeps the living set when the capacity is unchanged"""
        c = NrsDiffuseConfig()
        c.struct_size = C.sizeof(NrsDiffuseConfig) if struct_size is None else int(struct_size)
        c.capacity, c.seed = int(capacity), int(seed)
        c.tau_ta[:], c.tau_wc[:], c.tau_k[:] = [float(x) for x in tau_ta], [float(x) for x in tau_wc], [float(x) for x in tau_k]
        c.k_ta, c.k_wc = float(k_ta), float(k_wc)
        c.lifetime[:] = [float(x) for x in lifetime]
        c.k_buoyancy, c.k_drag = float(k_buoyancy), float(k_drag)
        c.spray_below, c.bubble_above, c.max_per_particle, c.reserved = int(spray_below), int(bubble_above), int(max_per_particle), int(reserved)
        self._chk(self.lib.nrs_diffuse_configure(self.h, C.byref(c)))

    def diffuse_step(self, dt=0.0):
        """one step of the diffuse particles on the current fluid state (nrs_diffuse_step; dt 0: the context's timestep); enqueues"""
        self._chk(self.lib.nrs_diffuse_step(self.h, float(dt)))

    def diffuse_count(self):
        """(alive, [spray, foam, bubble], dropped) of the diffuse set (nrs_diffuse_count; waits)"""
        a, d = C.c_uint64(0), C.c_uint64(0)
        k = (C.c_uint64 * 3)()
        self._chk(self.lib.nrs_diffuse_count(self.h, C.byref(a), k, C.byref(d)))
        return int(a.value), [int(x) for x in k], int(d.value)

    def diffuse_result(self, which):
        """one result on the host: (D, 4) SReal DIFFUSE_POS (w = lifetime) / DIFFUSE_VEL, (D,) uint32 DIFFUSE_KIND; per sorted fluid
        particle of the last step (N, 4) DIFFUSE_POTENTIALS / DIFFUSE_NORMALS, (N,) uint32 DIFFUSE_BIRTHS"""
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_diffuse_result(self.h, int(which), None, 0, C.byref(nbytes)))
        ints = which in (DIFFUSE_KIND, DIFFUSE_BIRTHS)
        dt = np.uint32 if ints else self.real
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_diffuse_result(self.h, int(which), _ptr(a), nbytes.value, None))
        return a if ints else a.reshape(-1, 4)

    def diffuse_device_ptr(self, which):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_diffuse_device_ptr(self.h, int(which), C.byref(p), C.byref(b)))
        return p.value, b.value

    def diffuse_upload(self, pos4, vel4):
        """replace the living diffuse set (nrs_diffuse_upload): (n, 4) positions with the lifetime in w, (n, 4) velocities"""
        pos4 = np.ascontiguousarray(pos4, dtype=self.real).reshape(-1, 4)
        vel4 = np.ascontiguousarray(vel4, dtype=self.real).reshape(-1, 4)
        assert len(pos4) == len(vel4)
        self._chk(self.lib.nrs_diffuse_upload(self.h, _ptr(pos4), _ptr(vel4), len(pos4)))

    def diffuse_release(self):
        self._chk(self.lib.nrs_diffuse_release(self.h))

    # ---- sources and sinks ----------------------------------------------------------------------------
    def emitter_set(self, slot, center=None, direction=None, half_extent=(0.0, 0.0), speed=0.0, spacing=0.0, shape=EMITTER_RECT,
                    enabled=True, max_particles=0):
        """store an emitter in `slot` (nrs_emitter_set), or remove it with center=None: layers of sites on a rectangle or disc through
        `center`, normal to `direction`, moving with `speed`; a layer is appended at the top of a step whenever speed * dt has
        accumulated one `spacing` (0: cbrt(particleMass / restDensity)); restarts the slot's accumulator and counts"""
        if center is None:
            self._chk(self.lib.nrs_emitter_set(self.h, int(slot), None))
            return
        e = NrsEmitter()
        e.shape, e.enabled, e.max_particles = int(shape), int(bool(enabled)), int(max_particles)
        he = list(np.broadcast_to(np.asarray(half_extent, np.float64), (2,)))
        e.center[:], e.direction[:], e.half_extent[:] = [float(x) for x in center], [float(x) for x in direction], [float(x) for x in he]
        e.speed, e.spacing = float(speed), float(spacing)
        self._chk(self.lib.nrs_emitter_set(self.h, int(slot), C.byref(e)))

    def emitter_get(self, slot):
        """(emitter as stored — a dict, direction normalised —, emitted, dropped) of a slot (nrs_emitter_get)"""
        e, a, d = NrsEmitter(), C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.nrs_emitter_get(self.h, int(slot), C.byref(e), C.byref(a), C.byref(d)))
        em = dict(shape=int(e.shape), enabled=bool(e.enabled), center=list(e.center), direction=list(e.direction),
                  half_extent=list(e.half_extent), speed=e.speed, spacing=e.spacing, max_particles=int(e.max_particles))
        return em, int(a.value), int(d.value)

    def emit_block(self, origin, spacing, dims, vel=(0.0, 0.0, 0.0)):
        """append the nodes of a lattice as fluid particles with velocity `vel` (nrs_emit_block): all or, above the capacity, none;
        returns how many were added"""
        L = self._lattice(origin, spacing, dims)
        v, added = (C.c_double * 3)(*[float(a) for a in vel]), C.c_uint64(0)
        self._chk(self.lib.nrs_emit_block(self.h, C.byref(L), v, C.byref(added)))
        return int(added.value)

    def emit_mesh(self, vertices, triangles, origin, spacing, dims, flags=MESH_INSIDE, dmin=0.0, dmax=float("inf"),
                  vel=(0.0, 0.0, 0.0)):
        """append the lattice nodes a rule selects against a triangle mesh (see mesh_particles) as fluid particles with velocity
        `vel` (nrs_emit_mesh): all or, above the capacity, none; returns how many were added"""
        M, keep = _mesh(vertices, triangles)
        L = self._lattice(origin, spacing, dims)
        R = _mesh_rule(flags, dmin, dmax)
        v, added = (C.c_double * 3)(*[float(a) for a in vel]), C.c_uint64(0)
        self._chk(self.lib.nrs_emit_mesh(self.h, C.byref(M), C.byref(L), C.byref(R), v, C.byref(added)))
        return int(added.value)

    def sinks_set(self, boxes=(), domain=False, interval=1, flags=None, nboxes=None, reserved=0):
        """kill volumes (nrs_sinks_set): boxes as rows (min xyz, max xyz), `domain`: also whatever leaves the grid box; culled before every
        interval-th step.  boxes=None clears the sinks."""
        if boxes is None:
            self._chk(self.lib.nrs_sinks_set(self.h, None))
            return
        b = np.asarray(boxes, np.float64).reshape(-1, 6)
        c = NrsSinkConfig()
        c.flags = (SINK_DOMAIN if domain else 0) if flags is None else int(flags)
        c.nboxes, c.interval, c.reserved = (len(b) if nboxes is None else int(nboxes)), int(interval), int(reserved)
        for i in range(min(len(b), MAX_SINK_BOXES)):
            c.boxes[i][:] = [float(x) for x in b[i]]
        self._chk(self.lib.nrs_sinks_set(self.h, C.byref(c)))

    def cull(self):
        """one cull now with the current sinks (nrs_cull; waits); returns how many particles were removed"""
        r = C.c_uint64(0)
        self._chk(self.lib.nrs_cull(self.h, C.byref(r)))
        return int(r.value)

    def sinks_count(self):
        """(particles removed, culls run) since the last sinks_set (nrs_sinks_count)"""
        r, c = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.nrs_sinks_count(self.h, C.byref(r), C.byref(c)))
        return int(r.value), int(c.value)

    # ---- particle identity and attributes -----------------------------------------------------------------
    def track_enable(self, flags=0):
        """number the particles now present 0 .. n-1 in the current order and start tracking (nrs_track_enable); TRACK_ATTR adds the
        attribute record; calling it again renumbers and resets"""
        self._chk(self.lib.nrs_track_enable(self.h, int(flags)))

    def track_disable(self):
        self._chk(self.lib.nrs_track_disable(self.h))

    def track_info(self):
        """(on, flags, next_id) (nrs_track_info)"""
        on, fl, nx = C.c_int(0), C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.nrs_track_info(self.h, C.byref(on), C.byref(fl), C.byref(nx)))
        return bool(on.value), int(fl.value), int(nx.value)

    def track_upload(self, which, src, first=0):
        """overwrite slots first .. first + len(src) of TRACK_ID / TRACK_BIRTH (uint32) or TRACK_ATTRIBUTE ((count, 4) SReal) (nrs_track_upload)"""
        if which == TRACK_ATTRIBUTE:
            a = np.ascontiguousarray(src, dtype=self.real).reshape(-1, 4)
        else:
            a = np.ascontiguousarray(src, dtype=np.uint32).reshape(-1)
        self._chk(self.lib.nrs_track_upload(self.h, int(which), _ptr(a) if len(a) else None, int(first), len(a)))

    def track_result(self, which):
        """one tracked array on the host, in the order of download(): (n,) uint32 ids / births, (n, 4) SReal records, or the (count,)
        uint32 slots of the last track_locate (nrs_track_result; waits)"""
        nbytes = C.c_uint64(0)
        self._chk(self.lib.nrs_track_result(self.h, int(which), None, 0, C.byref(nbytes)))
        dt = self.real if which == TRACK_ATTRIBUTE else np.uint32
        a = np.empty(nbytes.value // np.dtype(dt).itemsize, dtype=dt)
        if nbytes.value:
            self._chk(self.lib.nrs_track_result(self.h, int(which), _ptr(a), nbytes.value, None))
        return a.reshape(-1, 4) if which == TRACK_ATTRIBUTE else a

    def track_device_ptr(self, which):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.nrs_track_device_ptr(self.h, int(which), C.byref(p), C.byref(b)))
        return p.value, b.value

    def track_emit_value(self, slot, a):
        """the record given to the particles of emitter `slot`, or, slot -1, of emit_block, appended uploads and count growth"""
        v = (C.c_double * 4)(*[float(x) for x in a])
        self._chk(self.lib.nrs_track_emit_value(self.h, int(slot), v))

    def track_locate(self, first_id, count):
        """the slot of ids first_id .. first_id + count - 1 in the current order, TRACK_NONE where an id does not live
        (nrs_track_locate, then its result on the host)"""
        self._chk(self.lib.nrs_track_locate(self.h, int(first_id), int(count)))
        return self.track_result(TRACK_SLOT_OF)

    def track_diffuse(self, kappa, dt=0.0):
        """one explicit Euler step of da/dt = kappa_c lap a on the attribute record (nrs_track_diffuse; dt 0: the context's timestep)"""
        k = (C.c_double * 4)(*[float(x) for x in np.broadcast_to(np.asarray(kappa, np.float64), (4,))])
        self._chk(self.lib.nrs_track_diffuse(self.h, k, float(dt)))

    @property
    def n_owned(self):
        return int(self.lib.nrs_num_owned(self.h))

    def message_bytes(self, capacity):
        return int(self.lib.nrs_slab_message_bytes(int(capacity), 64 if self.double else 32))

    def max_density(self):
        v = C.c_double()
        self._chk(self.lib.nrs_max_density(self.h, C.byref(v)))
        return v.value

    def max_velocity(self):
        v = C.c_double()
        self._chk(self.lib.nrs_max_velocity(self.h, C.byref(v)))
        return v.value
