"""The host decisions of the field sampler (nereus_amd/csrc/nrs_host_sample.h) without a GPU, through a stand-alone program
(tests/host_sample_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): what is accepted, node counts and result sizes, every refusal, the cache rule, which result a field id
means.  And the ABI: the new symbols are declared, bound and exported.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, cmd, refusal, run

E_INVALID, E_STATE = -1, -4
D, G, V, N, W = 1, 2, 4, 8, 16
H = float(np.float32(0.0457))


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_sample_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_sample") / "host_sample"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_sample_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_sample"), SANITIZE)


def ok(ans):
    assert ans == ("rc", "0"), ans


def no(ans, code, part):
    c, msg = refusal(ans)
    assert c == code and part in msg, (ans, code, part)


# ---- fields, points, lattices -------------------------------------------------------------------------------------------------------
def check_fields(exe):
    good = [f | w for f in range(1, 16) for w in (0, W)]
    bad = [0, W, 32, 15 | 32, 64 | D, 1 << 31, 0xFFFFFFFF]
    ans = run(exe, [cmd("fields", f) for f in good + bad])
    for a in ans[:len(good)]:
        ok(a)
    no(ans[len(good)], E_INVALID, "no output")
    no(ans[len(good) + 1], E_INVALID, "no output")
    for a in ans[len(good) + 2:]:
        no(a, E_INVALID, "unknown bits")
    ans = run(exe, [cmd("points", 0, 0), cmd("points", 1, 0), cmd("points", 0, 5), cmd("points", 1, 5), cmd("points", 0, 2 ** 31),
                    cmd("points", 0, 2 ** 31 + 1)])
    ok(ans[0]), ok(ans[1]), ok(ans[2]), ok(ans[4])
    no(ans[3], E_INVALID, "points4 is NULL")
    no(ans[5], E_INVALID, "2^31")


def lattice(dims, spacing=(H / 2,) * 3, origin=(0.0, 0.0, 0.0)):
    return cmd("lattice", origin, spacing, dims)


def check_lattice(exe):
    cases = {(1, 1, 1): 1, (4, 4, 4): 64, (5, 4, 4): 80, (13, 7, 5): 455, (40, 40, 40): 64000, (2048, 2048, 512): 2 ** 31, (2 ** 31, 1, 1): 2 ** 31,
             (1, 3, 2 ** 29): 3 * 2 ** 29}
    ans = run(exe, [lattice(d) for d in cases])
    for a, (d, nodes) in zip(ans, cases.items()):
        assert a == ("nodes", str(nodes)), (d, a)
    # more than 2^31 nodes, however the factors are spread (no product wraps), and a dim of 0
    big = [(2048, 2048, 513), (2 ** 31 + 1, 1, 1), (65536, 65536, 1), (65536, 32768, 2), (0xFFFFFFFF,) * 3, (1, 0xFFFFFFFF, 0xFFFFFFFF), (3, 3, 2 ** 29)]
    for a in run(exe, [lattice(d) for d in big]):
        no(a, E_INVALID, "more than 2^31 nodes")
    for a in run(exe, [lattice(d) for d in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0))]):
        no(a, E_INVALID, "dim of 0")
    for bad in (0.0, -H, np.nan, np.inf, -np.inf):
        for axis in range(3):
            sp = [H, H, H]
            sp[axis] = bad
            no(run(exe, [lattice((2, 2, 2), sp)])[0], E_INVALID, "spacing")
    for bad in (np.nan, np.inf):
        no(run(exe, [lattice((2, 2, 2), origin=(0.0, bad, 0.0))])[0], E_INVALID, "origin")
    no(run(exe, ["nolattice"])[0], E_INVALID, "NULL")
    # tiny and huge spacings are numbers like any other
    assert run(exe, [lattice((2, 2, 2), (5e-324, 1e300, 1.0))])[0][0] == "nodes"


def check_bytes(exe):
    lines, want = [], []
    for m in (0, 1, 777, 2 ** 31):
        for prec, real in ((32, 4), (64, 8)):
            for f, size in ((D, real), (G, 4 * real), (V, 4 * real), (N, 4), (W, 0), (0, 0), (D | G, 0)):
                lines.append(cmd("bytes", f, m, prec))
                want.append(("bytes", str(size * m)))
    assert run(exe, lines) == want


# ---- refusals as a function of plain facts ---------------------------------------------------------------------------------------------
def refuse(mid=0, iisph=0, slab=0, grid=(16, 8, 8), cell=(H, H, H), h=H):
    return cmd("refuse", mid, iisph, slab, grid, cell, h)


def check_refusals(exe):
    ok(run(exe, [refuse()])[0])
    ok(run(exe, [refuse(grid=(4, 4, 4))])[0])
    ok(run(exe, [refuse(cell=(H, 2 * H, 1.5 * H))])[0])
    no(run(exe, [refuse(mid=1)])[0], E_STATE, "mid-update")
    no(run(exe, [refuse(iisph=1)])[0], E_STATE, "host-driven IISPH")
    no(run(exe, [refuse(slab=1)])[0], E_INVALID, "slab")
    no(run(exe, [refuse(slab=1, mid=1, iisph=1)])[0], E_INVALID, "slab")
    for axis in range(3):
        cell = [H, H, H]
        cell[axis] = float(np.nextafter(np.float64(H), 0.0))
        no(run(exe, [refuse(cell=cell)])[0], E_INVALID, "cellSize >= interactionRadius")
        cell[axis] = np.nan
        no(run(exe, [refuse(cell=cell)])[0], E_INVALID, "cellSize >= interactionRadius")
        for g in (1, 2):
            grid = [8, 8, 8]
            grid[axis] = g
            no(run(exe, [refuse(grid=grid)])[0], E_INVALID, "gridSize >= 4")
        for g in (5, 6, 12, 48):
            grid = [8, 8, 8]
            grid[axis] = g
            no(run(exe, [refuse(grid=grid)])[0], E_INVALID, "power-of-two")


# ---- the cache rule ------------------------------------------------------------------------------------------------------------------------
def check_cache(exe):
    seq = [((0, 1, 0, 1), 1), ((0, 1, 0, 1), 0), ((0, 1, 0, 1), 0),  # the same state does not rebuild
           ((1, 1, 0, 1), 1), ((1, 1, 0, 1), 0),                     # a step
           ((1, 2, 0, 1), 1), ((1, 2, 0, 1), 0),                     # an upload / nrs_set_num_particles
           ((1, 2, 1, 1), 1), ((1, 2, 1, 1), 0),                     # a grid change
           ((1, 2, 1, 2), 1), ((1, 2, 1, 2), 0),                     # a boundary change
           ((0, 1, 0, 1), 1)]                                        # an earlier key is another state too
    ans = run(exe, ["builds"] + [cmd("cache", *k) for k, _ in seq] + ["builds", "drop", "builds", cmd("cache", 0, 1, 0, 1), "builds"])
    assert ans[0] == ("builds", "0")
    builds = 0
    for a, (k, b) in zip(ans[1:], seq):
        builds += b
        assert a == ("build", "%d builds %d" % (b, builds)), (k, a)
    assert builds == 6
    tail = ans[1 + len(seq):]
    assert tail[0] == ("builds", "6") and tail[1] == ("ok", "")
    assert tail[2] == ("builds", "6")                                 # a release keeps the count ...
    assert tail[3] == ("build", "1 builds 7")                         # ... and the next call builds again, same key or not
    assert tail[4] == ("builds", "7")


def check_results(exe):
    ans = run(exe, [cmd("result", D, 32), cmd("last", 1, D | N, 777), cmd("result", D, 32), cmd("result", D, 64), cmd("result", N, 64), cmd("result", G, 32),
                    cmd("result", V, 32), cmd("result", W, 32), cmd("result", D | N, 32), cmd("last", 1, 15 | W, 0), cmd("result", V, 64), "drop",
                    cmd("result", D, 32)])
    no(ans[0], E_STATE, "no sample call yet")
    assert ans[2] == ("bytes", str(4 * 777)) and ans[3] == ("bytes", str(8 * 777)) and ans[4] == ("bytes", str(4 * 777))
    no(ans[5], E_STATE, "did not compute")
    no(ans[6], E_STATE, "did not compute")
    no(ans[7], E_INVALID, "one of")
    no(ans[8], E_INVALID, "one of")
    assert ans[10] == ("bytes", "0")
    no(ans[12], E_STATE, "no sample call yet")


def test_fields_points_lattices(plain):
    check_fields(plain)
    check_lattice(plain)
    check_bytes(plain)


def test_refusals(plain):
    check_refusals(plain)


def test_cache_rule_and_results(plain):
    check_cache(plain)
    check_results(plain)


def test_under_sanitizers(sanitized):
    check_fields(sanitized)
    check_lattice(sanitized)
    check_bytes(sanitized)
    check_refusals(sanitized)
    check_cache(sanitized)
    check_results(sanitized)


# ---- the ABI: declared, bound, exported ------------------------------------------------------------------------------------------------------
NEW = ["nrs_sample_points", "nrs_sample_lattice", "nrs_sample_result", "nrs_sample_device_ptr", "nrs_sample_release", "nrs_sample_builds"]


def test_sampler_abi_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(nrs_ctx \*ctx" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    flags = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_FIELD_[A-Z]+) = (\d+)", code))
    assert flags == {"NRS_FIELD_DENSITY": capi.FIELD_DENSITY, "NRS_FIELD_GRADIENT": capi.FIELD_GRADIENT, "NRS_FIELD_VELOCITY": capi.FIELD_VELOCITY,
                     "NRS_FIELD_COUNT": capi.FIELD_COUNT, "NRS_FIELD_WALLS": capi.FIELD_WALLS}
    assert (capi.FIELD_DENSITY, capi.FIELD_GRADIENT, capi.FIELD_VELOCITY, capi.FIELD_COUNT, capi.FIELD_WALLS) == (1, 2, 4, 8, 16)
    stats = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_STAT_[A-Z_]+) = (\d+)", text))
    assert max(stats.values()) == 11  # (the build count has an entry point of its own: the statistic ids are as they were)
    m = re.search(r"typedef struct nrs_lattice \{ double origin\[3\]; double spacing\[3\]; uint32_t dims\[3\]; uint32_t reserved; \} nrs_lattice;", code)
    assert m and __import__("ctypes").sizeof(capi.NrsLattice) == 64
    assert "came after nrs_version() 0.3 without a version change" in text.split("field sampling")[1][:200]
