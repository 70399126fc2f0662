"""The HIP-free parts of the surface extraction (nereus_amd/csrc/nrs_host_surface.h) without a GPU, through a stand-alone program
(tests/host_surface_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): what is accepted, every refusal, result sizes and routing; and the per-node and per-cell routines the kernels
call, driven serially over a lattice and compared with the numpy model (tests/surface_model.py) exactly — V, T, the vertex records bit
for bit, the triangles cell by cell.  And the ABI: the new symbols are declared, bound and exported.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import surface_model as sm
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, cmd, hx, refusal, run
from tests.test_surface_model_cpu import sphere, torus, two_blobs

E_INVALID, E_STATE = -1, -4
G, VEL, W = 1, 2, 4
MV, MT, MG, MVEL = 1, 2, 4, 8
H = float(np.float32(0.0457))


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_surface_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_surface") / "host_surface"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_surface_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_surface"), SANITIZE)


def ok(ans):
    assert ans == ("rc", "0"), ans


def no(ans, code, part):
    c, msg = refusal(ans)
    assert c == code and part in msg, (ans, code, part)


# ---- calls, lattices, sizes, routing ---------------------------------------------------------------------------------------------------
def lattice(dims, spacing=(H / 2,) * 3, origin=(0.0, 0.0, 0.0)):
    return cmd("lattice", origin, spacing, dims)


def check_calls(exe):
    for a in run(exe, [cmd("call", iso, f) for iso in (1e-300, 500.0, 1e300) for f in range(8)]):
        ok(a)
    for a in run(exe, [cmd("call", iso, 0) for iso in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf)]):
        no(a, E_INVALID, "iso")
    for a in run(exe, [cmd("call", 500.0, f) for f in (8, 16, 7 | 8, 1 << 31, 0xFFFFFFFF)]):
        no(a, E_INVALID, "unknown bits")
    assert run(exe, [cmd("fields", f) for f in range(8)]) == [("fields", str(1 | (2 if f & G else 0) | (4 if f & VEL else 0) | (16 if f & W else 0))) for f in range(8)]


def check_lattice(exe):
    cases = {(2, 2, 2): 8, (13, 7, 5): 455, (512, 512, 512): 2 ** 27, (2 ** 26, 2, 1 + 0): None, (2, 2, 2 ** 25): 2 ** 27}
    for d, nodes in cases.items():
        a = run(exe, [lattice(d)])[0]
        if nodes is None:
            no(a, E_INVALID, "dim >= 2")
        else:
            assert a == ("nodes", str(nodes)), (d, a)
    for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1)):
        no(run(exe, [lattice(d)])[0], E_INVALID, "dim >= 2")
    for d in ((512, 512, 513), (2, 2, 2 ** 25 + 1), (2 ** 27 + 1, 2, 2), (3, 3, 2 ** 24), (2048, 2048, 512)):
        no(run(exe, [lattice(d)])[0], E_INVALID, "2^27 nodes")
    # everything the sampler's lattice check refuses, with its texts
    for d in ((0, 4, 4), (4, 4, 0)):
        no(run(exe, [lattice(d)])[0], E_INVALID, "dim of 0")
    for d in ((2048, 2048, 513), (65536, 65536, 2), (0xFFFFFFFF,) * 3):
        no(run(exe, [lattice(d)])[0], E_INVALID, "more than 2^31 nodes")
    for bad in (0.0, -H, np.nan, np.inf):
        for axis in range(3):
            sp = [H, H, H]
            sp[axis] = bad
            no(run(exe, [lattice((2, 2, 2), sp)])[0], E_INVALID, "spacing")
    for bad in (np.nan, np.inf):
        no(run(exe, [lattice((2, 2, 2), origin=(0.0, bad, 0.0))])[0], E_INVALID, "origin")
    no(run(exe, ["nolattice"])[0], E_INVALID, "NULL")


def check_bytes_and_routing(exe):
    lines, want = [], []
    for V, T in ((0, 0), (7, 6), (1000, 1999), (7 * 2 ** 27, 12 * 2 ** 27)):
        for prec, vec4 in ((32, 16), (64, 32)):
            for w, size in ((MV, vec4 * V), (MG, vec4 * V), (MVEL, vec4 * V), (MT, 12 * T), (0, 0), (3, 0), (16, 0)):
                lines.append(cmd("bytes", w, V, T, prec))
                want.append(("bytes", str(size)))
    assert run(exe, lines) == want
    ans = run(exe, [cmd("result", MV, 32), cmd("last", 1, G, 70, 136), cmd("result", MV, 32), cmd("result", MV, 64), cmd("result", MT, 64),
                    cmd("result", MG, 32), cmd("result", MVEL, 32), cmd("result", 0, 32), cmd("result", MV | MT, 32), cmd("result", 16, 32),
                    cmd("last", 1, G | VEL | W, 0, 0), cmd("result", MVEL, 64), cmd("result", MT, 32), "drop", cmd("result", MV, 32),
                    cmd("result", 3, 32)])
    no(ans[0], E_STATE, "no surface extract yet")
    assert ans[2] == ("bytes", str(16 * 70)) and ans[3] == ("bytes", str(32 * 70)) and ans[4] == ("bytes", str(12 * 136))
    assert ans[5] == ("bytes", str(16 * 70))
    no(ans[6], E_STATE, "did not compute the velocity")
    for a in ans[7:10]:
        no(a, E_INVALID, "one of")
    assert ans[11] == ("bytes", "0") and ans[12] == ("bytes", "0")  # an empty surface: zero-byte results, not a refusal
    no(ans[14], E_STATE, "no surface extract yet")
    no(ans[15], E_INVALID, "one of")  # (what is wrong with the argument comes before what is wrong with the state)


# ---- the shared routines against the model --------------------------------------------------------------------------------------------
def run_mesh(exe, real, dens, origin, spacing, dims, iso):
    """the program's mesh of one lattice: (vertices (V, 4) in `real`, triangles (T, 3))"""
    prec = 64 if real == np.float64 else 32
    dens = np.ascontiguousarray(dens, dtype=real)
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    line = cmd("mesh", prec, origin, sp, dims, iso) + "".join(" " + hx(float(x)) for x in dens)
    ans = run(exe, [line])
    assert ans[0][0] == "mesh", ans[0]
    V, T = (int(x) for x in ans[0][1].split())
    assert len(ans) == 1 + V + T
    vert = np.array([[float.fromhex(t) for t in rest.split()] for w, rest in ans[1:1 + V]], np.float64).reshape(V, 4).astype(real)
    tri = np.array([[int(t) for t in rest.split()] for w, rest in ans[1 + V:]], np.uint32).reshape(T, 3)
    assert all(w == "v" for w, _ in ans[1:1 + V]) and all(w == "t" for w, _ in ans[1 + V:])
    return vert, tri


def against_model(exe, real, dens, origin, spacing, dims, iso, what):
    dens = np.ascontiguousarray(dens, dtype=real)
    vert, tri = run_mesh(exe, real, dens, origin, spacing, dims, iso)
    want = sm.extract(dens, origin, spacing, dims, iso, real)
    sm.compare(vert, tri, want, what=what)
    return vert, tri, want


def check_one_corner_inside(exe):
    """the eight one-corner-inside cases of a 2 x 2 x 2 lattice: corner 000 owns all seven vertices and sees six triangles (one per
    tet, all contain it); corner 111 is reached by seven edges of seven owners; the surface is open, every directed edge at most once"""
    for real in (np.float32, np.float64):
        for c in range(8):
            f = np.full(8, 0.25)
            f[c] = 2.0
            vert, tri, want = against_model(exe, real, f, (0.5, -1.0, 2.0), (0.9 * H, H, 1.1 * H), (2, 2, 2), 1.0, "corner %d" % c)
            sm.mesh_checks(vert, tri, closed=False)
            # the ends of the body diagonal lie on 3 axis edges, 3 face diagonals and the body diagonal, and in all six tets; every
            # other corner on 3 axis edges and one face diagonal, and in two tets
            assert (len(vert), len(tri)) == ((7, 6) if c in (0, 7) else (4, 2)), (c, len(vert), len(tri))
            assert len(np.unique(vert[:, :3], axis=0)) == len(vert)


def check_all_patterns(exe):
    """all 256 inside patterns of a 2 x 2 x 2 lattice (one cell, every case of every tet)"""
    rng = np.random.default_rng(7)
    for bits in range(256):
        f = rng.uniform(0.1, 0.9, 8)
        for c in range(8):
            if (bits >> c) & 1:
                f[c] += 1.0
        vert, tri, _ = against_model(exe, np.float64, f, (0.0, 0.0, 0.0), 1.0, (2, 2, 2), 1.0, "pattern %d" % bits)
        sm.mesh_checks(vert, tri, closed=False)


def check_lattices(exe):
    for real in (np.float32, np.float64):
        for name, field, chi in (("sphere", sphere, 2), ("two blobs", two_blobs, 4), ("torus", torus, 0)):
            f = field().astype(real)
            vert, tri, want = against_model(exe, real, f, (0, 0, 0), 1.0, (14, 14, 14), 1.0, name)
            assert sm.mesh_checks(vert, tri, closed=True, lattice_volume=13.0 ** 3)[0] == chi
        # nodes exactly at iso count as inside, t is 0 on their edges
        f = two_blobs().astype(real)
        assert (f == 1.0).sum() == 54
        vert, tri, want = against_model(exe, real, f, (0, 0, 0), 1.0, (14, 14, 14), 1.0, "at iso")
        assert (vert[:, 3] == 0).sum() > 54
        # odd, pairwise different dims, anisotropic spacing, an origin off zero, a surface cut by the boundary
        dims, sp, org = (9, 12, 7), (0.5, 0.25, 1.0), (-1.0, 2.0, 0.5)
        ax = sm.lattice_axes(org, sp, dims, np.float64)
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        f = (2.4 - np.sqrt((x + 0.5) ** 2 + (y - 3.4) ** 2 * 4 + (z - 3.4) ** 2 / 1.5)).ravel().astype(real)
        vert, tri, want = against_model(exe, real, f, org, sp, dims, 1.0, "cut")
        assert len(tri) > 50
        sm.mesh_checks(vert, tri, closed=False)


def test_calls_lattices_sizes_routing(plain):
    check_calls(plain)
    check_lattice(plain)
    check_bytes_and_routing(plain)


def test_one_corner_inside(plain):
    check_one_corner_inside(plain)


def test_all_patterns_of_a_cell(plain):
    check_all_patterns(plain)


def test_lattices_against_model(plain):
    check_lattices(plain)


def test_under_sanitizers(sanitized):
    check_calls(sanitized)
    check_lattice(sanitized)
    check_bytes_and_routing(sanitized)
    check_one_corner_inside(sanitized)
    check_all_patterns(sanitized)
    check_lattices(sanitized)


# ---- the ABI: declared, bound, exported ------------------------------------------------------------------------------------------------------
NEW = ["nrs_surface_extract", "nrs_surface_result", "nrs_surface_device_ptr", "nrs_surface_release"]


def test_surface_abi_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(nrs_ctx \*ctx" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    flags = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_SURFACE_[A-Z]+) = (\d+)", code))
    assert flags == {"NRS_SURFACE_GRADIENT": capi.SURFACE_GRADIENT, "NRS_SURFACE_VELOCITY": capi.SURFACE_VELOCITY, "NRS_SURFACE_WALLS": capi.SURFACE_WALLS}
    ids = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_MESH_[A-Z]+) = (\d+)", code))
    assert ids == {"NRS_MESH_VERTICES": capi.MESH_VERTICES, "NRS_MESH_TRIANGLES": capi.MESH_TRIANGLES, "NRS_MESH_GRADIENT": capi.MESH_GRADIENT,
                   "NRS_MESH_VELOCITY": capi.MESH_VELOCITY}
    assert (capi.SURFACE_GRADIENT, capi.SURFACE_VELOCITY, capi.SURFACE_WALLS) == (1, 2, 4)
    assert (capi.MESH_VERTICES, capi.MESH_TRIANGLES, capi.MESH_GRADIENT, capi.MESH_VELOCITY) == (1, 2, 4, 8)
    stats = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_STAT_[A-Z_]+) = (\d+)", text))
    assert max(stats.values()) == 11  # no new statistic id
    assert "came after nrs_version() 0.3 without a version change" in text.split("surface extraction")[1][:200]
