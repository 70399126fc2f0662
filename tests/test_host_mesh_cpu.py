"""The HIP-free parts of the mesh sampling (nereus_amd/csrc/nrs_host_mesh.h) without a GPU, through a stand-alone program
(tests/host_mesh_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): every refusal with its code and text; the gathered triangles; which halves of the field a rule needs and the
selection predicate against the numpy model (tests/mesh_model.py); the batch plan.  And the ABI: the new symbols are declared, bound
and exported, the pinned enums unchanged.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import mesh_model as mm
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, floats, hx, refusal, run

E_INVALID = -1


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + ["-I", os.path.join(ROOT, "include")] + extra + ["-o", out, os.path.join(ROOT, "tests", "host_mesh_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_mesh") / "host_mesh"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_mesh_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_mesh"), SANITIZE)


def no(ans, part):
    c, msg = refusal(ans)
    assert c == E_INVALID and part in msg and len(msg) > 0, (ans, part)


def mesh_line(v, t, has=1, nv=None, nt=None, give_v=True, give_t=True):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int64).reshape(-1, 3)
    out = ["mesh", str(int(has)), str(len(v) if nv is None else nv), str(len(t) if nt is None else nt)]
    out += [str(len(v) if give_v else 0)] + ([hx(x) for x in v.ravel()] if give_v else [])
    out += [str(len(t) if give_t else 0)] + ([str(int(x)) for x in t.ravel()] if give_t else [])
    return " ".join(out)


def rule_line(flags, dmin=0.0, dmax=np.inf, reserved=0, has=1):
    return "rule %d %d %d %s %s" % (has, flags, reserved, hx(dmin), hx(dmax))


V, T = mm.cube((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))


# ---- every refusal, with its code and text -----------------------------------------------------------------------------------------------------
def check_refusals(exe):
    assert run(exe, [mesh_line(V, T)]) == [("rc", "0")]
    no(run(exe, [mesh_line(V, T, has=0)])[0], "mesh is NULL")
    no(run(exe, [mesh_line(V, T, give_v=False)])[0], "vertices is NULL")
    no(run(exe, [mesh_line(V, T, give_t=False)])[0], "triangles is NULL")
    no(run(exe, [mesh_line(V, T, nv=0)])[0], "no vertices")
    no(run(exe, [mesh_line(V, T, nt=0)])[0], "no triangles")
    no(run(exe, [mesh_line(V, T, nt=1 << 31)])[0], "2^31 triangles")
    no(run(exe, [mesh_line(V, T, nt=(1 << 40) + 5)])[0], "2^31 triangles")
    bad = T.copy()
    bad[11, 2] = 8
    no(run(exe, [mesh_line(V, bad)])[0], "index is not below nv")
    bad[11, 2] = 0xFFFFFFFF
    no(run(exe, [mesh_line(V, bad)])[0], "index is not below nv")
    for x in (np.nan, np.inf, -np.inf):
        w = V.copy()
        w[7, 1] = x
        no(run(exe, [mesh_line(w, T)])[0], "not finite")
    # a triangle with two equal indices is a mesh like any other
    deg = T.copy()
    deg[3] = (1, 1, 5)
    assert run(exe, [mesh_line(V, deg)]) == [("rc", "0")]
    # rules
    for flags in (1, 2, 3, 5, 6, 7):
        assert run(exe, [rule_line(flags, 0.0, 0.5)])[0][0] == "r"
    no(run(exe, [rule_line(1, has=0)])[0], "rule is NULL")
    no(run(exe, [rule_line(0)])[0], "no side")
    no(run(exe, [rule_line(4)])[0], "no side")
    no(run(exe, [rule_line(8 | 1)])[0], "unknown bits")
    no(run(exe, [rule_line(0x80000001)])[0], "unknown bits")
    no(run(exe, [rule_line(1, reserved=1)])[0], "reserved")
    no(run(exe, [rule_line(1, dmin=-1e-300)])[0], "dmin")
    no(run(exe, [rule_line(1, dmin=np.nan)])[0], "dmin")
    no(run(exe, [rule_line(1, dmax=np.nan)])[0], "dmax is NaN")
    no(run(exe, [rule_line(1, dmin=0.5, dmax=0.25)])[0], "dmax below dmin")
    no(run(exe, [rule_line(1, dmin=np.inf, dmax=1.0)])[0], "dmax below dmin")
    assert run(exe, [rule_line(1, dmin=0.5, dmax=0.5)])[0][0] == "r"
    assert run(exe, [rule_line(1, dmin=np.inf, dmax=np.inf)])[0][0] == "r"
    # precision, SNAP into a context
    assert run(exe, ["precision 32", "precision 64"]) == [("rc", "0")] * 2
    for p in (0, 16, 33, 128):
        no(run(exe, ["precision %d" % p])[0], "precision must be 32 or 64")
    no(run(exe, ["snap"])[0], "NRS_MESH_SNAP")


def test_refusals(plain):
    check_refusals(plain)


def test_refusals_sanitized(sanitized):
    check_refusals(sanitized)


# ---- gathered triangles, the halves a rule needs, the predicate ----------------------------------------------------------------------------------
def check_decisions(exe):
    v, t = mm.icosphere(1, 0.3, (0.1, 0.2, 0.3))
    ans = run(exe, [mesh_line(v, t), "gather"])
    assert ans[0] == ("rc", "0") and ans[1][0] == "g"
    assert floats(ans[1][1]).tobytes() == v[t.astype(np.int64)].reshape(-1).tobytes()
    # (flags, dmin, dmax) -> (winding needed, distance needed)
    needs = [((1, 0.0, np.inf), (1, 0)), ((2, 0.0, np.inf), (1, 0)), ((3, 0.0, np.inf), (0, 1)), ((1, 0.02, np.inf), (1, 1)), ((1, 0.0, 0.3), (1, 1)),
             ((3, 0.0, 0.01), (0, 1)), ((1 | 4, 0.0, np.inf), (1, 1)), ((3 | 4, 0.0, 0.01), (0, 1))]
    for (flags, dmin, dmax), (uw, ud) in needs:
        word, rest = run(exe, [rule_line(flags, dmin, dmax)])[0]
        tok = rest.split()
        assert word == "r" and (int(tok[0]), int(tok[1])) == (uw, ud), (flags, dmin, dmax, rest)
        assert floats(" ".join(tok[2:])).tobytes() == np.array([np.float64(dmin) * np.float64(dmin), np.float64(dmax) * np.float64(dmax)]).tobytes()
    # the predicate against the model's, on values around every threshold
    s = 0.02
    ws = [0.0, 0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0), 1.0, -0.3, 2.0]
    ds = [0.0, s * s, np.nextafter(s * s, 0.0), np.nextafter(s * s, 1.0), (s / 2) * (s / 2), np.nextafter((s / 2) * (s / 2), 1.0), 1.0, np.inf]
    rules = [(1, s, np.inf), (2, s, np.inf), (3, 0.0, s / 2), (1, 0.0, np.inf), (2, 0.0, s / 2), (3, 0.0, np.inf), (1 | 4, 0.0, s / 2), (3, s / 2, s)]
    lines, want = [], []
    for flags, dmin, dmax in rules:
        f = dict(winding=np.repeat(ws, len(ds)), dist2=np.tile(ds, len(ws)))
        want += mm.selected(f, flags, dmin, dmax).astype(int).tolist()
        lines += ["sel %d %s %s %s %s" % (flags, hx(dmin), hx(dmax), hx(w), hx(d)) for w, d in zip(f["winding"], f["dist2"])]
    got = [int(rest) for word, rest in run(exe, lines)]
    assert got == want and 0 < sum(want) < len(want)


def test_decisions(plain):
    check_decisions(plain)


def test_decisions_sanitized(sanitized):
    check_decisions(sanitized)


# ---- the batch plan: the ranges cover [0, N) once and in order, none above 2^22 -----------------------------------------------------------------------
def check_plan(exe):
    assert mm.header_constant("nrs_host_mesh.h", "MESH_BATCH") == mm.BATCH == 1 << 22
    sizes = [1, 255, 1 << 22, (1 << 22) + 1, 4300800, (1 << 31) - 1, 1 << 31]
    for n, (word, rest) in zip(sizes, run(exe, ["plan %d" % n for n in sizes])):
        tok = [int(x) for x in rest.split()]
        assert word == "plan" and tok[0] == -(-n // mm.BATCH) and len(tok) == 1 + 2 * tok[0]
        first, count = np.array(tok[1::2]), np.array(tok[2::2])
        assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == n
        assert (count >= 1).all() and (count <= mm.BATCH).all()


def test_plan(plain):
    check_plan(plain)


def test_plan_sanitized(sanitized):
    check_plan(sanitized)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
NEW = ["nrs_mesh_field", "nrs_mesh_particles", "nrs_emit_mesh"]


def test_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.NrsMesh) == 32 and C.sizeof(capi.NrsMeshRule) == 24
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_[A-Z0-9_]+) = (\d+)", code))
    flags = dict((k, int(v)) for k, v in re.findall(r"#define (NRS_MESH_[A-Z]+) (\d+)u", code))
    assert flags == {"NRS_MESH_INSIDE": capi.MESH_INSIDE, "NRS_MESH_OUTSIDE": capi.MESH_OUTSIDE, "NRS_MESH_SNAP": capi.MESH_SNAP}
    assert (capi.MESH_INSIDE, capi.MESH_OUTSIDE, capi.MESH_SNAP) == (1, 2, 4)
    assert (mm.INSIDE, mm.OUTSIDE, mm.SNAP) == (1, 2, 4)
    # the surface extraction's results keep their names and values next to the new flags
    assert (enums["NRS_MESH_VERTICES"], enums["NRS_MESH_TRIANGLES"]) == (capi.MESH_VERTICES, capi.MESH_TRIANGLES) == (1, 2)
    # the pinned enums did not grow
    assert sorted(v for k, v in enums.items() if k.startswith("NRS_STAT_")) == list(range(12))
    assert enums["NRS_STAGE_COUNT"] == 16
    assert (enums["NRS_MAX_EMITTERS"], enums["NRS_MAX_SINK_BOXES"]) == (16, 16)
