"""The host decisions and the per-particle finishing routine of the anisotropic surface reconstruction
(nereus_amd/csrc/nrs_host_aniso.h) without a GPU, through a stand-alone program (tests/host_aniso_main.cpp) built with the host compiler,
plain and under -fsanitize=address,undefined (a host program of its own: nothing is preloaded): every acceptance and refusal, sizes and
routing; the finishing routine — the code the kernel runs — against the numpy model (tests/aniso_model.py) on covariances of every
rank and multiplicity and at the clamp boundaries.  And the ABI: the new symbols are declared, bound and exported.

The bar of the finishing routine.  The inputs are the same numbers on both sides (sums representable in the build's real type R), so the
difference is the rounding of the routine in R.  Forming C = S / Sw - mu mu^T costs at most 4 eps (|S / Sw| + |mu|^2), which is
<= 8 eps |C| for the cases here (|mu|^2 <= |C|); the cyclic Jacobi is backward stable, its decomposition is exact for C + E with
|E| <= ~10 eps |C| after its 18 to 24 rotations; so the eigenvalues move by <= ~18 eps s1.  A clamped eigenvalue max(s_k, s1 / k_r) is
>= s1 / k_r, so its relative change is <= 18 k_r eps; a_k = support st_k / cbrt(st_1 st_2 st_3) moves relatively by at most twice
that, and so does 1 / a_k.  G is a matrix function of C with these eigenvalue maps (equal eigenvalues give equal a_k: the arbitrary basis
of an eigenspace cancels), and |G|_F support <= sqrt(3) k_r^(2/3) ~ 4.4 for k_r = 4: |G - G_model|_F support <= ~160 k_r eps.  The
bar is 200 k_r eps (fp32 9.5e-5, fp64 1.8e-13 for k_r = 4), below the caps of 1e-3 / 1e-10 above which a difference means an
unconverged eigen solve.  Centre and weight: a handful of roundings each, 32 eps relative (the centre relative to h).
Measured here (x86-64, g++ -O3): fp32 G 9.1e-7, fp64 G 2.4e-15.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import aniso_model as am
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, cmd, floats, refusal, run

E_INVALID, E_STATE = -1, -4
H = float(np.float32(0.0457))
NAN, INF = float("nan"), float("inf")
GRAD, VEL, WALLS = 1, 2, 4


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_aniso_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_aniso") / "host_aniso"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_aniso_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_aniso"), SANITIZE)


def ok(ans):
    assert ans == ("rc", "0"), ans


def no(ans, code, part):
    c, msg = refusal(ans)
    assert c == code and part in msg, (ans, code, part)


# ---- the configuration ------------------------------------------------------------------------------------------------------------------
def config(support=0.0, lam=0.9, k_r=4.0, k_n=0.5, n_eps=25, reserved=0, null=0, h=H):
    return cmd("config", null, support, lam, k_r, k_n, n_eps, reserved, h)


def check_config(exe):
    good = [config(null=1), config(null=1, support=NAN, reserved=7), config(), config(support=H), config(support=1.5 * H), config(support=1e-9),
            config(lam=0.0), config(lam=1.0), config(k_r=1.0), config(k_r=1e6), config(k_n=1.0), config(k_n=1e-6), config(n_eps=0),
            config(n_eps=2 ** 32 - 1)]
    ans = run(exe, good)
    for a in ans:
        assert a[0] == "cfg", a
    for a in ans[:4]:  # NULL (whatever the struct holds), support 0 and support h: the defaults
        v = a[1].split()
        np.testing.assert_array_equal(floats(" ".join(v[:4])), [H, 0.9, 4.0, 0.5])
        assert v[4] == "25"
    assert floats(ans[4][1].rsplit(" ", 1)[0])[0] == 1.5 * H and ans[13][1].split()[4] == str(2 ** 32 - 1)
    bad = [(config(support=np.nextafter(1.5 * H, 1)), "support"), (config(support=-H), "support"), (config(support=2 * H), "support"),
           (config(lam=-1e-9), "lambda"), (config(lam=np.nextafter(1.0, 2)), "lambda"), (config(k_r=np.nextafter(1.0, 0)), "k_r"), (config(k_r=0.0), "k_r"),
           (config(k_r=-4.0), "k_r"), (config(k_n=0.0), "k_n"), (config(k_n=np.nextafter(1.0, 2)), "k_n"), (config(k_n=-0.5), "k_n"),
           (config(reserved=1), "reserved"), (config(h=0.0), "interactionRadius"), (config(null=1, h=-1.0), "interactionRadius"),
           (config(null=1, h=NAN), "interactionRadius")]
    bad += [(config(**{k: v}), "non-finite") for k in ("support", "lam", "k_r", "k_n") for v in (NAN, INF, -INF)]
    for a, (_, part) in zip(run(exe, [b[0] for b in bad]), bad):
        no(a, E_INVALID, part)


# ---- refusals of a context, of an extract ----------------------------------------------------------------------------------------------------
def facts(mid=0, iisph=0, slab=0, grid=(16, 16, 16), cell=(H, H, H), h=H):
    return cmd("refuse", mid, iisph, slab, grid, cell, h)


def check_refusals(exe):
    ans = run(exe, [facts(), facts(grid=(8, 8, 8)), facts(grid=(8, 64, 1024)), facts(cell=(2 * H, H, 3 * H))])
    for a in ans:
        ok(a)
    # the sampler's refusals, word for word
    ans = run(exe, [facts(slab=1), facts(mid=1), facts(iisph=1), facts(h=0.0), facts(cell=(0.9 * H, H, H)), facts(grid=(12, 16, 16)),
                    facts(grid=(16, 2, 16))])
    no(ans[0], E_INVALID, "slab context"), no(ans[1], E_STATE, "mid-update"), no(ans[2], E_STATE, "IISPH"), no(ans[3], E_INVALID, "interactionRadius > 0")
    no(ans[4], E_INVALID, "cellSize >= interactionRadius"), no(ans[5], E_INVALID, "power-of-two"), no(ans[6], E_INVALID, "gridSize >= 4")
    # its own: five cells of a row need eight
    for g in ((4, 16, 16), (16, 4, 16), (16, 16, 4), (4, 4, 4)):
        no(run(exe, [facts(grid=g)])[0], E_INVALID, "gridSize >= 8")
    ans = run(exe, [cmd("extract", 0.5, f) for f in (0, GRAD, VEL, GRAD | VEL)])
    assert [a for a in ans] == [("fields", str(f)) for f in (1, 1 | 2, 1 | 4, 1 | 2 | 4)]
    ans = run(exe, [cmd("extract", 0.5, WALLS), cmd("extract", 0.5, WALLS | GRAD), cmd("extract", 0.5, 8), cmd("extract", 0.0, 0), cmd("extract", -1.0, 0),
                    cmd("extract", NAN, 0), cmd("extract", INF, 0)])
    no(ans[0], E_INVALID, "no wall term"), no(ans[1], E_INVALID, "no wall term"), no(ans[2], E_INVALID, "unknown bits")
    for a in ans[3:]:
        no(a, E_INVALID, "iso must be finite and > 0")


# ---- sizes and routing -------------------------------------------------------------------------------------------------------------------------
def check_results(exe):
    want = {(1, 32): 16, (1, 64): 32, (2, 32): 32, (2, 64): 64, (4, 32): 4, (4, 64): 4, (8, 32): 4, (8, 64): 4}
    for n in (0, 1, 1080, 2 ** 31):
        ans = run(exe, [cmd("bytes", w, n, p) for (w, p) in want])
        assert ans == [("bytes", str(v * n)) for v in want.values()]
    assert run(exe, [cmd("bytes", w, 10, 32) for w in (0, 3, 16)]) == [("bytes", "0")] * 3
    ans = run(exe, [cmd("result", 1, 32), cmd("last", 1, 1080), cmd("result", 1, 32), cmd("result", 2, 64), cmd("result", 4, 32), cmd("result", 8, 64),
                    cmd("result", 0, 32), cmd("result", 3, 32), cmd("result", 16, 32), cmd("last", 1, 0), cmd("result", 2, 32), cmd("last", 0, 5),
                    cmd("result", 8, 32), cmd("result", 5, 32)])
    no(ans[0], E_STATE, "no nrs_aniso_build yet")
    assert ans[2:6] == [("bytes", "17280"), ("bytes", "69120"), ("bytes", "4320"), ("bytes", "4320")]
    for a in ans[6:9]:
        no(a, E_INVALID, "which must be one of")
    assert ans[10] == ("bytes", "0")
    no(ans[12], E_STATE, "no nrs_aniso_build yet")
    no(ans[13], E_INVALID, "which must be one of")  # (a bad id is refused before the state)


# ---- the finishing routine ------------------------------------------------------------------------------------------------------------------------
def rot(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q


def covariance_cases():
    """name -> (eigenvalues, rotation, mu, count, config overrides); lengths in units of h"""
    s = (0.6 * H) ** 2
    c = {
        "zero": ((0, 0, 0), np.eye(3), (0, 0, 0), 40, {}),
        "rank1": ((s, 0, 0), rot(1), (0, 0, 0), 40, {}),
        "rank1_axis": ((0, s, 0), np.eye(3), (0, 0, 0), 40, {}),
        "rank2": ((s, 0.5 * s, 0), rot(2), (0.1 * H, 0, 0), 40, {}),
        "two_equal_large": ((s, s, 0.1 * s), rot(3), (0, 0.05 * H, 0.02 * H), 40, {}),
        "two_equal_small": ((s, 0.3 * s, 0.3 * s), rot(4), (0, 0, 0), 40, {}),
        "three_equal": ((s, s, s), rot(5), (0.01 * H, 0.01 * H, 0.01 * H), 40, {}),
        "three_equal_diagonal": ((s, s, s), np.eye(3), (0, 0, 0), 40, {}),
        "generic": ((s, 0.6 * s, 0.4 * s), rot(6), (0.2 * H, -0.1 * H, 0.05 * H), 60, {}),
        "nearly_equal": ((s, s * (1 - 1e-5), s * (1 - 2e-5)), rot(7), (0, 0, 0), 40, {}),
        "at_the_ratio": ((s, s / 4, s / 4), rot(8), (0, 0, 0), 40, {}),
        "count_below_n_eps": ((s, 0.1 * s, 0.1 * s), rot(9), (0, 0, 0), 24, {}),
        "count_at_n_eps": ((s, 0.1 * s, 0.1 * s), rot(9), (0, 0, 0), 25, {}),
        "axis_clamped": ((s, 0, 0), rot(10), (0, 0, 0), 40, dict(support=1.5 * H)),       # a1 = 1.5 h 16^(1/3) > 3 h / 2
        "axis_not_clamped": ((s, 0, 0), rot(10), (0, 0, 0), 40, dict(support=0.5 * H)),
        "shift_clamped": ((s, 0.5 * s, 0.2 * s), rot(11), (0.5 * H, 0.4 * H, 0), 40, dict(lam=1.0)),   # |lambda mu| = 0.64 h > h / 2
        "shift_just_below": ((s, 0.5 * s, 0.2 * s), rot(11), (0.49 * H, 0, 0), 40, dict(lam=1.0)),
        "shift_just_above": ((s, 0.5 * s, 0.2 * s), rot(11), (0.51 * H, 0, 0), 40, dict(lam=1.0)),
        "lambda_zero": ((s, 0.5 * s, 0.2 * s), rot(12), (0.3 * H, 0.2 * H, 0), 40, dict(lam=0.0)),
        "k_r_one": ((s, 0.5 * s, 0.2 * s), rot(13), (0, 0, 0), 40, dict(k_r=1.0)),
        "no_neighbour": ((0, 0, 0), np.eye(3), (0, 0, 0), 0, {}),
    }
    return c


def finish_case(real, ev, q, mu, count, over, rng):
    """the command line of one case with sums representable in `real`, and the model's record of the same sums"""
    cfg = am.config(H, **over)
    sw = float(real(max(count, 1) * 0.55))
    C = q @ np.diag(np.asarray(ev, np.float64)) @ q.T
    mu = np.asarray(mu, np.float64)
    M = (sw * mu).astype(real).astype(np.float64)
    S = (sw * (C + np.outer(mu, mu))).astype(real).astype(np.float64)
    S = (S + S.T) / 2
    D = float(real(max(count, 1) * 0.4 * (2 * H) ** 6))
    x = rng.uniform(-1, 1, 3).astype(real).astype(np.float64)
    line = cmd("finish", 64 if real == np.float64 else 32, H, cfg["support"], cfg["lam"], cfg["k_r"], cfg["k_n"], cfg["n_eps"], x, count,
               0.0 if not count else sw, M, S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2], D)
    r = float(real(2) * real(H))
    want = am.finish(np.array([sw if count else 0.0]), M[None], S[None], np.array([D]), np.array([count]), x[None], H, r, cfg)
    return line, want, cfg


def check_finish(exe, real):
    eps = float(np.finfo(real).eps)
    rng = np.random.default_rng(17)
    worst = dict(G=0.0, center=0.0, weight=0.0)
    cases = covariance_cases()
    built = {name: finish_case(real, *c, rng) for name, c in cases.items()}
    ans = run(exe, [b[0] for b in built.values()])
    for a, (name, (line, want, cfg)) in zip(ans, built.items()):
        assert a[0] == "rec", (name, a)
        v = floats(a[1])
        c, bound, g, weight, axes = v[:3], v[3], v[4:10], v[10], v[11:14]
        G = np.array([[g[0], g[1], g[2]], [g[1], g[3], g[4]], [g[2], g[4], g[5]]])
        if name == "no_neighbour":
            assert not G.any() and weight == 0 and bound == 0
            np.testing.assert_array_equal(c, want["center"][0])
            continue
        eG = float(np.linalg.norm(G - want["G"][0])) * cfg["support"]
        ec = float(np.abs(c - want["center"][0]).max()) / H
        ew = abs(weight - want["weight"][0]) / want["weight"][0]
        worst = dict(G=max(worst["G"], eG), center=max(worst["center"], ec), weight=max(worst["weight"], ew))
        assert eG <= 200 * cfg["k_r"] * eps, (name, eG)
        # (the centre is x + delta with |x| up to 1: its rounding is relative to |x|, not to h)
        assert ec <= 32 * eps * max(1.0, 1.0 / H), (name, ec)
        assert ew <= 32 * eps + 6 * 200 * cfg["k_r"] * eps, (name, ew)
        np.testing.assert_allclose(np.sort(axes), np.sort(want["axes"][0]), rtol=400 * cfg["k_r"] * eps, err_msg=name)
        assert abs(bound - axes.max()) == 0 and bound <= float(real(1.5 * H)) * (1 + eps), name
    # what the cases are there for
    w = {k: v[1] for k, v in built.items()}
    assert np.allclose(w["zero"]["axes"], 0.5 * H) and np.allclose(w["count_below_n_eps"]["axes"], 0.5 * H)
    # (a needle with support h: the short axes are h / 4 * 16^(1/3) = 0.63 h, the long one would be 2.52 h and stops at 3 h / 2)
    for name in ("count_at_n_eps", "rank1"):
        assert np.isclose(w[name]["axes"].min(), 0.25 * H * 16 ** (1 / 3)) and w[name]["axes"].max() == 1.5 * H
    assert np.isclose(w["axis_not_clamped"]["axes"].max() / w["axis_not_clamped"]["axes"].min(), 4.0) and np.isclose(np.prod(w["axis_not_clamped"]["axes"]), (H / 2) ** 3)
    assert w["axis_clamped"]["bound"][0] == 1.5 * H and w["axis_not_clamped"]["bound"][0] < 1.5 * H
    assert np.allclose(w["three_equal"]["axes"], H) and np.allclose(w["k_r_one"]["axes"], H)
    print("finishing routine, %s: max |G - G_model|_F support %.3g, centre / h %.3g, weight (relative) %.3g" % (np.dtype(real).name, worst["G"], worst["center"], worst["weight"]))
    return worst


def check_eigen(exe, real):
    """the fixed-length Jacobi converges: U^T A U is diagonal and U orthonormal to rounding, on every multiplicity and on scales from 1e-12 to 1e6"""
    eps = float(np.finfo(real).eps)
    rng = np.random.default_rng(23)
    mats = []
    for k in range(40):
        q = rot(100 + k)
        ev = [(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0), (3, 2, 1), (1, 1 - 1e-6, 1 - 2e-6), (1, 1e-7, 1e-14), (2, 2, 1)][k % 8]
        mats.append((q @ np.diag(np.array(ev, np.float64) * 10.0 ** rng.integers(-12, 7)) @ q.T).astype(real).astype(np.float64))
    mats.append(np.diag([3.0, 1.0, 2.0]))
    mats.append(np.array([[1e-3, 1e-30, 0], [1e-30, 1e-3, 0], [0, 0, 1e-3]]) if real == np.float64 else np.array([[1e-3, 1e-20, 0], [1e-20, 1e-3, 0], [0, 0, 1e-3]]))
    ans = run(exe, [cmd("eigen", 64 if real == np.float64 else 32, (a + a.T)[np.triu_indices(3)] / 2) for a in mats])
    for a, A in zip(ans, mats):
        v = floats(a[1])
        lam, U = v[:3], v[3:].reshape(3, 3)
        A = (A + A.T) / 2
        scale = max(np.abs(A).max(), 1e-300)
        assert np.abs(U.T @ U - np.eye(3)).max() <= 64 * eps
        assert np.abs(U @ np.diag(lam) @ U.T - A).max() <= 64 * eps * scale, (A, lam)
        np.testing.assert_allclose(np.sort(lam), np.linalg.eigvalsh(A), atol=64 * eps * scale, rtol=0)


def check_cloud(exe, real):
    """sums and finishing routine together on a random cloud: the candidate routine in R against the model's membership and float64 sums"""
    eps = float(np.finfo(real).eps)
    rng = np.random.default_rng(29)
    x = rng.uniform(0, 5 * H, (200, 3)).astype(real)
    want = am.records(x, H, real)
    for i in (0, 57, 199):
        p = np.roll(x, -i, axis=0)
        a = run(exe, [cmd("cloud", 64 if real == np.float64 else 32, H, H, 0.9, 4.0, 0.5, 25, len(p), p.astype(np.float64))])[0]
        rec, count = a[1].rsplit(" ", 1)
        v = floats(rec)
        g = v[4:10]
        G = np.array([[g[0], g[1], g[2]], [g[1], g[3], g[4]], [g[2], g[4], g[5]]])
        assert int(count) == want["count"][i] and want["count"][i] >= 25
        # (about count terms per sum on top of the finishing routine's own budget)
        assert np.linalg.norm(G - want["G"][i]) * H <= (200 + 8 * want["count"][i]) * 4.0 * eps
        assert abs(v[10] - want["weight"][i]) / want["weight"][i] <= (32 + 6 * (200 + 8 * want["count"][i]) * 4.0) * eps
        assert np.abs(v[:3] - want["center"][i]).max() / H <= (32 + 2 * want["count"][i]) * eps * 5.0


def test_configurations(plain):
    check_config(plain)


def test_refusals_sizes_and_routing(plain):
    check_refusals(plain)
    check_results(plain)


@pytest.mark.parametrize("real", [np.float32, np.float64], ids=["f32", "f64"])
def test_finishing_routine_against_the_model(plain, real):
    check_eigen(plain, real)
    worst = check_finish(plain, real)
    assert worst["G"] <= (1e-3 if real == np.float32 else 1e-10)
    check_cloud(plain, real)


def test_under_sanitizers(sanitized):
    check_config(sanitized)
    check_refusals(sanitized)
    check_results(sanitized)
    for real in (np.float32, np.float64):
        check_eigen(sanitized, real)
        check_finish(sanitized, real)
        check_cloud(sanitized, real)


# ---- the ABI: declared, bound, exported ------------------------------------------------------------------------------------------------------
NEW = ["nrs_aniso_build", "nrs_aniso_result", "nrs_aniso_device_ptr", "nrs_aniso_release", "nrs_surface_extract_aniso"]


def test_aniso_abi_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(nrs_ctx \*ctx" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    ids = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_ANISO_[A-Z]+) = (\d+)", code))
    assert ids == {"NRS_ANISO_CENTER": capi.ANISO_CENTER, "NRS_ANISO_G": capi.ANISO_G, "NRS_ANISO_COUNT": capi.ANISO_COUNT, "NRS_ANISO_INDEX": capi.ANISO_INDEX}
    assert re.search(r"typedef struct nrs_aniso_config \{ double support, lambda, k_r, k_n; uint32_t n_eps, reserved; \} nrs_aniso_config;", code)
    assert ctypes.sizeof(capi.NrsAnisoConfig) == 40
    assert code.rstrip().endswith("#endif") and code.index("nrs_surface_extract_aniso") > code.index("nrs_max_velocity")  # (appended: nothing before it moved)
