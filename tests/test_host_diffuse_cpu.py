"""The HIP-free parts of the diffuse particles (nereus_amd/csrc/nrs_host_diffuse.h) without a GPU, through a stand-alone program
(tests/host_diffuse_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): what is accepted, every refusal with its text, result sizes and routing; and the hash, the clamp, the birth
count, the birth and the advection routines the kernels call, driven serially and compared with the numpy model
(tests/diffuse_model.py) bit for bit.  And the ABI: the new symbols are declared, bound and exported, the statistic ids unchanged.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import diffuse_model as dm
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, hx, refusal, run

E_INVALID, E_STATE = -1, -4
H = float(np.float32(0.0457))
SIZE = C.sizeof(capi.NrsDiffuseConfig)
POS, VEL, KIND, POT, BIRTHS, NORMALS = range(6)


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + ["-I", os.path.join(ROOT, "include")] + extra + ["-o", out, os.path.join(ROOT, "tests", "host_diffuse_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_diffuse") / "host_diffuse"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_diffuse_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_diffuse"), SANITIZE)


def line(name, *vals):
    """a command line: Python ints travel as decimals, everything else as hex floats"""
    out = [name]
    for v in vals:
        for x in (v if isinstance(v, (list, tuple, np.ndarray)) else [v]):
            out.append(str(int(x)) if isinstance(x, (int, np.integer, bool)) else hx(float(x)))
    return " ".join(out)


def ok(ans):
    assert ans == ("rc", "0"), ans


def no(ans, code, part):
    c, msg = refusal(ans)
    assert c == code and part in msg, (ans, code, part)


def cfg_line(c, struct_size=SIZE, reserved=0):
    return line("cfg", struct_size, c["capacity"], c["seed"], c["tau_ta"], c["tau_wc"], c["tau_k"], c["k_ta"], c["k_wc"], c["lifetime"], c["k_buoyancy"],
                c["k_drag"], c["spray_below"], c["bubble_above"], c["max_per_particle"], reserved)


# ---- configurations, calls, sizes, routing -----------------------------------------------------------------------------------------------
def check_config(exe):
    assert SIZE == 128
    good = dm.config(capacity=1000)
    for c in (good, dm.config(capacity=1), dm.config(capacity=1 << 30), dm.config(capacity=5, lifetime=(0.0, 0.0)), dm.config(capacity=5, k_drag=0.0),
              dm.config(capacity=5, k_drag=1.0, max_per_particle=1024, spray_below=0, bubble_above=0, seed=2 ** 64 - 1, k_ta=0.0, k_wc=0.0)):
        ok(run(exe, [cfg_line(c)])[0])
    bad = [(dict(capacity=0), "capacity of 0"), (dict(capacity=(1 << 30) + 1), "capacity above 2^30"),
           (dict(tau_ta=(1.0, 1.0)), "tau_ta"), (dict(tau_ta=(2.0, 1.0)), "tau_ta"), (dict(tau_wc=(np.nan, 1.0)), "tau_wc"),
           (dict(tau_wc=(0.0, np.inf)), "tau_wc"), (dict(tau_k=(3.0, -3.0)), "tau_k"), (dict(k_ta=-1.0), "k_ta"), (dict(k_ta=np.nan), "k_ta"),
           (dict(k_wc=np.inf), "k_wc"), (dict(lifetime=(-1.0, 2.0)), "lifetime"), (dict(lifetime=(3.0, 2.0)), "lifetime"),
           (dict(lifetime=(0.0, np.inf)), "lifetime"), (dict(k_buoyancy=np.nan), "k_buoyancy"), (dict(k_drag=-0.1), "k_drag"),
           (dict(k_drag=1.5), "k_drag"), (dict(k_drag=np.nan), "k_drag"), (dict(max_per_particle=0), "max_per_particle"),
           (dict(max_per_particle=1025), "max_per_particle")]
    for kw, part in bad:
        c = dict(good)
        c.update(kw)
        no(run(exe, [cfg_line(c)])[0], E_INVALID, part)
    no(run(exe, [cfg_line(good, struct_size=SIZE - 8)])[0], E_INVALID, "struct_size")
    no(run(exe, [cfg_line(good, struct_size=0)])[0], E_INVALID, "struct_size")
    no(run(exe, [cfg_line(good, reserved=1)])[0], E_INVALID, "reserved")
    no(run(exe, ["nocfg"])[0], E_INVALID, "NULL")
    # the size is named before the fields
    c = dict(good, capacity=0)
    no(run(exe, [cfg_line(c, struct_size=4)])[0], E_INVALID, "struct_size")


def facts(slab=0, mid=0, iisph=0, grid=(64, 16, 16), cell=(H, H, H), h=H, configured=1):
    return line("refusal", slab, mid, iisph, list(grid), list(cell), h, configured)


def check_refusals(exe):
    for dt in (0.0, 1e-3, 1e300, 5e-324):
        ok(run(exe, [line("dt", dt)])[0])
    for dt in (np.nan, -1e-3, -np.inf, np.inf, -5e-324):
        no(run(exe, [line("dt", dt)])[0], E_INVALID, "dt must be finite and >= 0")
    ok(run(exe, [facts()])[0])
    ok(run(exe, [facts(grid=(4, 4, 4), cell=(2 * H, H, 3 * H))])[0])
    no(run(exe, [facts(configured=0)])[0], E_STATE, "before nrs_diffuse_configure")
    no(run(exe, [facts(slab=1)])[0], E_INVALID, "slab context")
    no(run(exe, [facts(slab=1, configured=0, mid=1)])[0], E_INVALID, "slab context")
    no(run(exe, [facts(mid=1)])[0], E_STATE, "mid-update after nrs_step_partial")
    no(run(exe, [facts(mid=1, configured=0)])[0], E_STATE, "before nrs_diffuse_configure")
    no(run(exe, [facts(iisph=1)])[0], E_STATE, "host-driven IISPH step")
    no(run(exe, [facts(h=0.0)])[0], E_INVALID, "interactionRadius > 0")
    no(run(exe, [facts(cell=(H, 0.99 * H, H))])[0], E_INVALID, "cellSize >= interactionRadius")
    no(run(exe, [facts(grid=(64, 2, 16))])[0], E_INVALID, "gridSize >= 4")
    no(run(exe, [facts(grid=(64, 16, 12))])[0], E_INVALID, "power-of-two gridSize")
    ok(run(exe, [line("fits", 2 ** 21, 1024)])[0])
    no(run(exe, [line("fits", 2 ** 21 + 1, 1024)])[0], E_INVALID, "above 2^31")
    ok(run(exe, [line("upload", 1, 1, 10, 10)])[0])
    ok(run(exe, [line("upload", 0, 0, 0, 10)])[0])
    no(run(exe, [line("upload", 1, 1, 11, 10)])[0], E_INVALID, "more particles than the configured capacity")
    no(run(exe, [line("upload", 0, 1, 3, 10)])[0], E_INVALID, "NULL array")
    no(run(exe, [line("upload", 1, 0, 3, 10)])[0], E_INVALID, "NULL array")


def check_bytes_and_routing(exe):
    lines, want = [], []
    for D, N in ((0, 0), (7, 1080), (2 ** 30, 2 ** 31)):
        for prec, vec4 in ((32, 16), (64, 32)):
            for w, size in ((POS, vec4 * D), (VEL, vec4 * D), (KIND, 4 * D), (POT, vec4 * N), (NORMALS, vec4 * N), (BIRTHS, 4 * N), (6, 0), (99, 0)):
                lines.append(line("bytes", w, D, N, prec))
                want.append(("bytes", str(size)))
    assert run(exe, lines) == want
    route = lambda conf, stepped, N, w, alive, prec: line("route", conf, stepped, N, w, alive, prec)
    ans = run(exe, [route(0, 0, 0, POS, 0, 32), route(1, 0, 0, POS, 5, 32), route(1, 0, 0, KIND, 5, 64), route(1, 0, 0, POT, 5, 32),
                    route(1, 1, 1080, POT, 5, 32), route(1, 1, 1080, BIRTHS, 5, 64), route(1, 1, 1080, NORMALS, 0, 64), route(1, 1, 0, VEL, 0, 32),
                    route(0, 0, 0, 6, 0, 32), route(1, 1, 10, 6, 3, 32), route(1, 1, 10, 0xFFFFFFFF, 3, 32)])
    no(ans[0], E_STATE, "before nrs_diffuse_configure")
    assert ans[1] == ("bytes", "80") and ans[2] == ("bytes", "20")   # the living set (an upload) before any step
    no(ans[3], E_STATE, "no diffuse step yet")
    assert ans[4] == ("bytes", str(16 * 1080)) and ans[5] == ("bytes", str(4 * 1080)) and ans[6] == ("bytes", str(32 * 1080))
    assert ans[7] == ("bytes", "0")  # an empty set: zero bytes, not a refusal
    for a in ans[8:]:
        no(a, E_INVALID, "one of")  # (what is wrong with the argument comes before what is wrong with the state)


# ---- the shared routines against the model, bit for bit ------------------------------------------------------------------------------------------
def vals(ans, word):
    assert ans[0] == word, ans
    return ans[1].split()


def check_hash_and_draws(exe):
    rng = np.random.default_rng(3)
    seed = [0, 1, 2012, 2 ** 64 - 1] + [int(x) for x in rng.integers(0, 2 ** 63, 20)]
    step = [0, 1, 9, 2 ** 40] + [int(x) for x in rng.integers(0, 10 ** 6, 20)]
    slot = [0, 1, 2 ** 32 - 1, 1079] + [int(x) for x in rng.integers(0, 2 ** 32, 20)]
    draw = [0, 1, 40, 2 ** 32 - 1] + [int(x) for x in rng.integers(0, 10 ** 4, 20)]
    got = run(exe, [line("hash", *t) for t in zip(seed, step, slot, draw)])
    want = dm.hash64(np.array(seed, np.uint64), np.array(step, np.uint64), np.array(slot, np.uint64), np.array(draw, np.uint64))
    assert [int(vals(a, "hash")[0]) for a in got] == [int(x) for x in want]
    for prec, real in ((32, np.float32), (64, np.float64)):
        got = run(exe, [line("uniform", prec, *t) for t in zip(seed, step, slot, draw)])
        u = dm.uniform(np.array(seed, np.uint64), np.array(step, np.uint64), np.array(slot, np.uint64), np.array(draw, np.uint64), real)
        assert [float.fromhex(vals(a, "u")[0]) for a in got] == [float(x) for x in u]
        x = rng.uniform(-1, 3, 50).astype(real)
        got = run(exe, [line("clamp", prec, float(v), 0.25, 1.75) for v in x] + [line("clamp", prec, np.nan, 0.25, 1.75)])
        want = dm._clamp(np.append(x, real(np.nan)), 0.25, 1.75, real)
        assert [float.fromhex(vals(a, "c")[0]) for a in got] == [float(v) for v in want]
        assert want[-1] == 1 and want.min() == 0 and want.max() == 1
        c = dm.config(capacity=10, max_per_particle=3)
        rate = np.concatenate((rng.uniform(0, 5000, 60), [0.0, np.nan, np.inf, 1e30, 2999.9999])).astype(real)
        uu = np.concatenate((rng.integers(0, 2 ** 24, 60) * 2.0 ** -24, [0.999, 0.5, 0.5, 0.5, 0.0])).astype(real)
        got = run(exe, [cfg_line(c)] + [line("births", prec, float(r), 1e-3, float(q)) for r, q in zip(rate, uu)])
        want = dm.births_count(c, rate, real(1e-3), uu, real)
        assert [int(vals(a, "n")[0]) for a in got[1:]] == [int(v) for v in want]
        assert set(want.tolist()) == {0, 1, 2, 3}


def check_births(exe):
    rng = np.random.default_rng(4)
    for prec, real in ((32, np.float32), (64, np.float64)):
        c = dm.config(capacity=10, seed=77, lifetime=(0.5, 2.5))
        m = 200
        xi = rng.uniform(-1, 1, (m, 3)).astype(real)
        vi = rng.normal(0, 1, (m, 3)).astype(real)
        vi[0] = 0                      # no direction: the frame is (x, y), the height 0
        vi[1] = (0, 0, 3)              # along an axis
        vi[2] = (1, 1, 1)              # a three-way tie
        vi[3] = (0.5, -0.5, 2)         # a two-way tie
        vi[4] = (1e-30, 0, 0)          # length() underflows to 0 in float
        slot = rng.integers(0, 5000, m)
        k = rng.integers(0, 8, m)
        step = 5
        got = run(exe, [cfg_line(c)] + [line("birth", prec, step, int(slot[q]), int(k[q]), xi[q].astype(np.float64), vi[q].astype(np.float64), 0.02, 1e-3)
                                        for q in range(m)])
        x, v, life = dm.birth_rule(c, step, slot, k, xi, vi, 0.02, 1e-3, real)
        want = np.concatenate((x, life[:, None], v), axis=1)
        have = np.array([[float.fromhex(t) for t in vals(a, "b")] for a in got[1:]]).astype(real)
        assert have.tobytes() == want.tobytes(), np.abs(have.astype(np.float64) - want).max()
        assert np.all(life >= 0.5) and np.all(life <= 2.5)
        r = np.linalg.norm((v - vi).astype(np.float64), axis=1)
        assert r.max() <= 0.02 * (1 + 1e-5) and r.max() > 0.015  # the radial offset stays inside the cylinder


def check_advection(exe):
    rng = np.random.default_rng(5)
    for prec, real in ((32, np.float32), (64, np.float64)):
        c = dm.config(capacity=10, spray_below=5, bubble_above=6, k_buoyancy=2.0, k_drag=0.5)
        m = 300
        lo, hi = np.array((-0.1, -0.1, -0.1), real), np.array((0.9, 0.5, 0.7), real)
        x = rng.uniform(-0.1, 0.9, (m, 3)).astype(real) * np.array((1, 0.6, 0.8), real)
        v = rng.normal(0, 1, (m, 3)).astype(real)
        vt = rng.normal(0, 1, (m, 3)).astype(real)
        life = rng.uniform(0.0, 3e-3, m).astype(real)
        n = rng.integers(0, 12, m)
        x[0], v[0], n[0] = (0.8999, 0.2, 0.2), (2.0, 0, 0), 0          # leaves through the high x face
        x[1], v[1], n[1] = (-0.0999, 0.2, 0.2), (-2.0, 0, 0), 0        # ... the low one
        x[2], v[2], n[2], life[2] = (0.2, 0.2, 0.2), (np.inf, 0, 0), 0, 1.0   # non-finite after the move
        life[3], n[3] = 1e-3, 5                                           # foam whose lifetime reaches exactly 0
        life[4], n[4] = 0.0, 0                                            # spray with no lifetime left
        g = np.array((0, -9.81, 0), real)
        got = run(exe, [cfg_line(c)] + [line("advect", prec, x[q].astype(np.float64), v[q].astype(np.float64), float(life[q]), vt[q].astype(np.float64),
                                             int(n[q]), g.astype(np.float64), 1e-3, lo.astype(np.float64), hi.astype(np.float64)) for q in range(m)])
        xn, vn, ln, kind, alive = dm.advect_rule(c, x, v, life, vt, n, g, 1e-3, lo, hi, real)
        want = np.concatenate((xn, ln[:, None], vn), axis=1)
        rows = [vals(a, "a") for a in got[1:]]
        assert [int(r[0]) for r in rows] == [int(a) for a in alive] and [int(r[1]) for r in rows] == [int(q) for q in kind]
        have = np.array([[float.fromhex(t) for t in r[2:]] for r in rows]).astype(real)
        assert have.tobytes() == want.tobytes()
        assert not alive[:5].any() and set(kind.tolist()) == {0, 1, 2} and 0.2 < alive.mean() < 0.95


def test_configurations_and_refusals(plain):
    check_config(plain)
    check_refusals(plain)
    check_bytes_and_routing(plain)


def test_hash_clamp_and_birth_count_match_model(plain):
    check_hash_and_draws(plain)


def test_births_match_model(plain):
    check_births(plain)


def test_advection_matches_model(plain):
    check_advection(plain)


def test_under_sanitizers(sanitized):
    check_config(sanitized)
    check_refusals(sanitized)
    check_bytes_and_routing(sanitized)
    check_hash_and_draws(sanitized)
    check_births(sanitized)
    check_advection(sanitized)


# ---- the ABI: declared, bound, exported ------------------------------------------------------------------------------------------------------
NEW = ["nrs_diffuse_configure", "nrs_diffuse_step", "nrs_diffuse_count", "nrs_diffuse_result", "nrs_diffuse_device_ptr", "nrs_diffuse_upload",
       "nrs_diffuse_release"]


def test_diffuse_abi_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(nrs_ctx \*ctx" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    ids = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_DIFFUSE_[A-Z]+) = (\d+)", code))
    assert ids == {"NRS_DIFFUSE_POS": capi.DIFFUSE_POS, "NRS_DIFFUSE_VEL": capi.DIFFUSE_VEL, "NRS_DIFFUSE_KIND": capi.DIFFUSE_KIND,
                   "NRS_DIFFUSE_POTENTIALS": capi.DIFFUSE_POTENTIALS, "NRS_DIFFUSE_BIRTHS": capi.DIFFUSE_BIRTHS, "NRS_DIFFUSE_NORMALS": capi.DIFFUSE_NORMALS}
    assert sorted(ids.values()) == list(range(6))
    # the struct of the binding is the header's, field by field
    body = re.search(r"typedef struct nrs_diffuse_config \{(.*?)\} nrs_diffuse_config;", code, flags=re.S).group(1)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [f[0] for f in capi.NrsDiffuseConfig._fields_]
    assert C.sizeof(capi.NrsDiffuseConfig) == 128
    stats = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_STAT_[A-Z_]+) = (\d+)", text))
    assert max(stats.values()) == 11  # no new statistic id
    assert "came after nrs_version() 0.3 without a version change" in text.split("diffuse particles")[1][:200]
    assert "-g_i / |g_i|" in text.split("diffuse particles")[1]  # the orientation of the normal is stated
