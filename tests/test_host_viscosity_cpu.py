"""The HIP-free parts of the implicit viscosity solve (nereus_amd/csrc/nrs_host_viscosity.h) without a GPU, through a stand-alone
program (tests/host_viscosity_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of
its own: nothing is preloaded): every acceptance and refusal of the settings with its text, the inputs of the exit rule, the slot rr
alternates between, the buffer sizes and the guards of alpha and beta.  And the ABI: the two symbols are declared, bound and exported.
"""
import os
import re
import subprocess

import pytest

from nereus_amd import capi
from tests.test_host_inflow_cpu import line, no
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, floats, run

E_INVALID, E_STATE = -1, -4
NEW = ["nrs_dfsph_set_viscosity", "nrs_dfsph_viscosity_info"]
NAN, INF = float("nan"), float("inf")


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_viscosity_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_visc") / "host_visc"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_visc_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_visc"), SANITIZE)


def _set(nu, nub, tol, mn, mx, moving=0):
    return line("set", float(nu), float(nub), float(tol), int(mn), int(mx), int(moving))


def _accepted(ans):
    word, rest = ans
    assert word == "set", ans
    t = rest.split()
    return dict(on=int(t[0]), nu=float.fromhex(t[1]), nub=float.fromhex(t[2]), tol=float.fromhex(t[3]), mn=int(t[4]), mx=int(t[5]),
                fixed=int(t[6]), cap=int(t[7]))


def check_settings(exe):
    # accepted: the ends of the ranges, fixed mode, the default cap, off
    a = _accepted(run(exe, [_set(1.0, 0.5, 1e-3, 2, 40)])[0])
    assert a == dict(on=1, nu=1.0, nub=0.5, tol=1e-3, mn=2, mx=40, fixed=0, cap=40)
    a = _accepted(run(exe, [_set(0.01, 0.0, 1e-8, 0, 0)])[0])
    assert a["on"] == 1 and a["fixed"] == 0 and a["cap"] == 100 and a["mn"] == 0
    a = _accepted(run(exe, [_set(100.0, 0.0, 0.0, 3, 0)])[0])
    assert a["fixed"] == 1 and a["cap"] == 3
    a = _accepted(run(exe, [_set(1.0, 0.0, 0.0, 3, 3)])[0])
    assert a["fixed"] == 1 and a["cap"] == 3
    a = _accepted(run(exe, [_set(1.0, 0.0, 0.999999, 5, 5)])[0])
    assert a["cap"] == 5
    a = _accepted(run(exe, [_set(0.0, 7.0, 1e-3, 1, 0)])[0])           # off: the wall friction goes with it
    assert a["on"] == 0 and a["nub"] == 0.0
    a = _accepted(run(exe, [_set(0.0, 1.0, 1e-3, 1, 0, moving=1)])[0])  # off is accepted on a context with moving bodies
    assert a["on"] == 0
    a = _accepted(run(exe, [_set(1.0, 0.0, 1e-3, 1, 0, moving=1)])[0])  # slip walls may move
    assert a["on"] == 1 and a["nub"] == 0.0
    # refused, each with its text
    for nu, nub in ((-1.0, 0.0), (NAN, 0.0), (INF, 0.0), (1.0, -1e-9), (1.0, NAN), (1.0, INF), (-INF, 0.0)):
        no(run(exe, [_set(nu, nub, 1e-3, 1, 0)])[0], E_INVALID, "finite and >= 0")
    for tol in (-1e-12, 1.0, 2.0, NAN, INF):
        no(run(exe, [_set(1.0, 0.0, tol, 1, 0)])[0], E_INVALID, "tolerance must be in [0, 1)")
    no(run(exe, [_set(1.0, 0.0, 0.0, 0, 0)])[0], E_INVALID, "min_iters >= 1")
    no(run(exe, [_set(1.0, 0.0, 0.0, 0, 5)])[0], E_INVALID, "min_iters >= 1")
    no(run(exe, [_set(1.0, 0.0, 1e-3, 4, 3)])[0], E_INVALID, "max_iters below min_iters")
    no(run(exe, [_set(1.0, 0.0, 0.0, 4, 3)])[0], E_INVALID, "max_iters below min_iters")
    no(run(exe, [_set(1.0, 0.25, 1e-3, 1, 0, moving=1)])[0], E_STATE, "boundary bodies move")
    # a refused set changes nothing
    got = run(exe, [_set(2.0, 0.5, 1e-2, 2, 9), _set(-1.0, 0.0, 1e-3, 1, 0), _set(3.0, 1.0, 1e-3, 1, 0, moving=1), line("measure", 1.0, 4.0)])
    assert _accepted(got[0])["nu"] == 2.0 and got[1][0] == "rc" and got[2][0] == "rc"
    assert floats(got[3][1])[0] == 1.0 - 1e-2 * 1e-2 * 4.0


def check_exit_inputs_sizes_guards(exe):
    # the measure: rr - tol^2 bb, the loop stops on <= 0
    got = run(exe, [_set(1.0, 0.0, 1e-3, 1, 0), line("measure", 1e-6, 1.0), line("measure", 1.0000001e-6, 1.0), line("measure", 0.0, 0.0),
                    line("measure", NAN, 1.0)])
    m = [floats(g[1])[0] for g in got[1:]]
    assert m[0] <= 0.0 and m[1] > 0.0 and m[2] == 0.0 and not (m[3] <= 0.0)
    assert [int(g[1]) for g in run(exe, ["slot 0", "slot 1", "slot 2", "slot 3", "slot 4294967295"])] == [2, 3, 2, 3, 3]
    assert run(exe, ["sizes 1080 4", "sizes 1080 8", "sizes 0 4", "sizes 4096000 4"]) == [
        ("sizes", "17280 4320 64"), ("sizes", "34560 8640 64"), ("sizes", "0 0 64"), ("sizes", "65536000 16384000 64")]
    # the guards: alpha = 0 when p.q <= 0 or not a number, beta = 0 when rr = 0
    a = [floats(g[1])[0] for g in run(exe, [line("alpha", 2.0, 4.0), line("alpha", 2.0, 0.0), line("alpha", 2.0, -1.0), line("alpha", 2.0, NAN),
                                            line("alpha", 0.0, 0.0), line("alpha", 0.0, 3.0)])]
    assert a == [0.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    b = [floats(g[1])[0] for g in run(exe, [line("beta", 1.0, 4.0), line("beta", 1.0, 0.0), line("beta", 0.0, 0.0), line("beta", 0.0, 2.0),
                                            line("beta", 1.0, -1.0)])]
    assert b == [0.25, 0.0, 0.0, 0.0, 0.0]


def test_settings(plain):
    check_settings(plain)


def test_exit_inputs_sizes_guards(plain):
    check_exit_inputs_sizes_guards(plain)


def test_sanitized(sanitized):
    check_settings(sanitized)
    check_exit_inputs_sizes_guards(sanitized)


def test_symbols_header_and_binding():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+nrs_dfsph_set_viscosity\s*\(\s*nrs_ctx\s*\*\s*ctx\s*,\s*double\s+nu\s*,\s*double\s+nu_boundary\s*,\s*double\s+tolerance\s*,"
                     r"\s*uint32_t\s+min_iters\s*,\s*uint32_t\s+max_iters\s*\)\s*;", code)
    assert re.search(r"\bint\s+nrs_dfsph_viscosity_info\s*\(\s*nrs_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*on\s*,\s*uint32_t\s*\*\s*iterations\s*,"
                     r"\s*double\s*\*\s*residual\s*,\s*double\s*\*\s*rhs_norm\s*\)\s*;", code)
    assert re.search(r"\bNRS_STAGE_COUNT\s*=\s*16\b", code)
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert hasattr(capi.Solver, "dfsph_set_viscosity") and hasattr(capi.Solver, "dfsph_viscosity_info")
    assert lib.nrs_dfsph_set_viscosity(None, 1.0, 0.0, 1e-3, 1, 0) == -1   # a NULL context is refused before anything else
    assert lib.nrs_dfsph_viscosity_info(None, None, None, None, None) == -1
