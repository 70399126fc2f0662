"""The boundary tables and bodies of a context, call by call, against a recording (tests/golden/boundary_catalogue.json, written by
tests/golden/make_boundary_catalogue.py on the MI355X from the commit before the boundary state moved out of the context into
nrs_boundary_tables.h), and what a refused nrs_set_boundaries leaves behind.

Scene: small_dam_break((20, 16, 14)) with its five-face box: 4,480 particles, a grid of 64 columns in x.  Contexts: fp32 Müller SESPH (near
bits and wall workgroups live), fp64 Monaghan IISPH (no list kernels, so no near bits), fp32 Müller DFSPH (the wall-velocity term).
At eight moments — the rest build, the rebuild after a shifted origin, a body assignment (the box floor as body 1), the posed build
twice, a teleport, clearing the bodies while displaced, another set of boundary particles, and on a second context the rebuild for a
slab's cell-table window — every NRS_ARR_B_* id is asked: the code and text when refused, else the byte count and a SHA-256 of the
bytes (NRS_ARR_B_CELL_END only in the cells whose start is not empty: it is defined only there).  With them nrs_get_params as bytes
and, after every stepping moment, the fluid's positions and velocities.  On the 64-column grid the narrowest window an IISPH slab (halo
8) can ask for is the whole grid, and DFSPH has no slabs: the recording holds what those two contexts answer instead."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from nereus_amd import capi
from tests.common import small_dam_break

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary_catalogue.json")
LATTICE = (20, 16, 14)
# case: solver, fp64, kernel set, the slab (lo, hi, halo) of the second context
CASES = {"sesph-f32-muller": (capi.SESPH, False, capi.MULLER, (0, 8, 2)),
         "iisph-f64-monaghan": (capi.IISPH, True, capi.MONAGHAN, (0, 16, 8)),
         "dfsph-f32-muller": (capi.DFSPH, False, capi.MULLER, (0, 8, 2))}
B_IDS = {"b_hash": 12, "b_index": 13, "b_cell_start": 14, "b_cell_end": 15, "b_sorted": 16, "b_body": 35}
EMPTY = 0xFFFFFFFF
_scenes = {}


def scene(case):
    """(params, scene) of the case, built once"""
    if case not in _scenes:
        solver, double, kernel_set, _ = CASES[case]
        _scenes[case] = small_dam_break(LATTICE, solver=solver, double=double, kernel_set=kernel_set)
    return _scenes[case]


def context(case):
    """a context on the case's scene after nrs_set_boundaries(update_grid = 1), with fixed iteration counts"""
    solver, double, kernel_set, _ = CASES[case]
    p, sc = scene(case)
    s = capi.Solver(p, len(sc["pos"]), solver=solver, double=double, kernel_set=kernel_set)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    if solver == capi.IISPH:
        s.set_max_iterations(4)
    if solver == capi.DFSPH:
        s.dfsph_configure(0.0, 3, 0.0, 3, 1)
    return s


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _size(s, which):
    """(rc, byte count) of an array id, asked with a null destination: nothing is copied"""
    b = C.c_uint64(0)
    rc = s.lib.nrs_get_array(s.h, which, None, 0, C.byref(b))
    return rc, b.value


def tables(s):
    """{name: {"rc", "msg"} | {"bytes", "sha256"}} of the NRS_ARR_B_* ids"""
    raw, out = {}, {}
    for name, which in B_IDS.items():
        rc, nbytes = _size(s, which)
        if rc:
            out[name] = {"rc": rc, "msg": s.lib.nrs_last_error().decode()}
            continue
        a = np.zeros(nbytes // 4, np.uint32)
        if nbytes:
            s._chk(s.lib.nrs_get_array(s.h, which, a.ctypes.data_as(C.c_void_p), nbytes, None))
        raw[name] = a
        out[name] = {"bytes": nbytes}
    if "b_cell_end" in raw and "b_cell_start" in raw and raw["b_cell_end"].size:
        raw["b_cell_end"] = np.where(raw["b_cell_start"] != EMPTY, raw["b_cell_end"], 0).astype(np.uint32)
    for name, a in raw.items():
        out[name]["sha256"] = _sha(a)
    return out


def moment(s, stepped):
    o = {"tables": tables(s), "params": s.params.tobytes().hex()}
    if stepped:
        pos, vel = s.download()
        o["pos"], o["vel"] = _sha(pos), _sha(vel)
    return o


def catalogue(case):
    """{moment: what moment() collects} of one case"""
    _, _, _, slab = CASES[case]
    p, sc = scene(case)
    bi, vbi = sc["bi"], sc["vbi"]
    out = {}
    s = context(case)
    try:
        out["1-set_boundaries"] = moment(s, False)
        q = s.params.copy()
        q["worldOrigin"][0][:3] = q["worldOrigin"][0][:3] - np.array([0.013, 0.021, 0.008])
        s.set_params(q)
        out["2-set_params"] = moment(s, False)
        body_of = (bi[:, 1] == 0).astype(np.uint32)     # the box floor (y = 0) is body 1
        assert 0 < body_of.sum() < len(body_of)
        s.set_boundary_bodies(body_of, 2)
        out["3-set_boundary_bodies"] = moment(s, False)
        s.set_body_velocity(1, (0.3, 0.5, -0.2), (0.0, 0.0, 0.2))
        s.step(2)
        out["4-velocity-2-steps"] = moment(s, True)
        x, _ = s.body_pose(1)
        s.set_body_pose(1, x + np.array([0.01, 0.02, 0.0]), (1.0, 0.0, 0.0, 0.001))
        s.step(1)
        out["5-pose-1-step"] = moment(s, True)
        s.set_boundary_bodies(None, 0)
        out["6-cleared"] = moment(s, False)
        s.step(1)
        out["6-cleared-1-step"] = moment(s, True)
        more = bi[:37].copy()
        more[:, :3] += bi.dtype.type(0.01)
        s.set_boundaries(np.concatenate([bi, more]), np.concatenate([vbi, vbi[:37]]), update_grid=False)
        out["7-set_boundaries-again"] = moment(s, False)
    finally:
        s.close()
    s = context(case)
    try:
        rc = s.lib.nrs_slab_configure(s.h, *slab)
        out["8-slab_configure"] = moment(s, False)
        out["8-slab_configure"]["call"] = {"rc": rc, "msg": s.lib.nrs_last_error().decode() if rc else ""}
    finally:
        s.close()
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_boundary_catalogue_equals_recording(hip_lib, case):
    with open(FIXTURE) as f:
        want = json.load(f)[case]
    got = json.loads(json.dumps(catalogue(case)))
    assert sorted(got) == sorted(want)
    for m in sorted(want):
        assert sorted(got[m]) == sorted(want[m]), m
        for k in sorted(want[m]):
            if k != "tables":
                assert got[m][k] == want[m][k], "%s %s: %s differs from the recording" % (case, m, k)
                continue
            assert sorted(got[m][k]) == sorted(want[m][k]), m
            for name in sorted(want[m][k]):
                assert got[m][k][name] == want[m][k][name], "%s %s %s: got %s want %s" % (case, m, name, got[m][k][name], want[m][k][name])


def test_refused_set_boundaries_changes_nothing(hip_lib):
    """A grid of more than 2^31 cells is refused before anything is stored: the parameters, the size of every boundary array and the
    bodies are those of a twin that was never asked, and so is the run that follows."""
    case = "sesph-f32-muller"
    p, sc = scene(case)
    bi, vbi = sc["bi"], sc["vbi"]
    body_of = (bi[:, 1] == 0).astype(np.uint32)
    a, b = context(case), context(case)
    try:
        a.set_boundary_bodies(body_of, 2)
        b.set_boundary_bodies(body_of, 2)
        far = np.ones((2, 4), bi.dtype)
        far[0, :3] = -0.5                          # (outside the box: the origin of the refused grid is not the old one)
        far[1, :3] = -0.5 + 1e4 / np.sqrt(3.0)     # 10^4 m away along the diagonal: 2^17 cells on every axis
        big, vbig = np.concatenate([bi, far]), np.concatenate([vbi, vbi[:2]])
        rc = a.lib.nrs_set_boundaries(a.h, big.ctypes.data_as(C.c_void_p), vbig.ctypes.data_as(C.c_void_p), len(big), 1)
        assert rc == -1 and a.lib.nrs_last_error().decode() == "grid from boundary AABB exceeds 2^31 cells"
        # host-only answers first: nothing below this block may run on tables that a refused call resized
        assert a.params.tobytes() == b.params.tobytes()
        for name, which in B_IDS.items():
            assert _size(a, which) == _size(b, which), name
        for u, v in zip(a.body_pose(1), b.body_pose(1)):
            np.testing.assert_array_equal(u, v)
        a.step(3)
        b.step(3)
        for u, v in zip(a.download(), b.download()):
            np.testing.assert_array_equal(u, v)
    finally:
        a.close()
        b.close()
