"""The library's HIP-free host components (nereus_amd/csrc/nrs_host_bodies.h, nrs_host_settings.h) without a GPU: a stand-alone
program (tests/host_parts_main.cpp) built with the host compiler, -ffp-contract=off as the library is, fed commands on stdin.

  * the pose integration against tests/bodies_model.advance, for 1 and for 50 consecutive steps.  x: 1 ulp per component per step
    (the same two IEEE operations on both sides; measured: identical).  q: the largest component difference these cases give,
    measured where this test was written, is 0 after one step and 2.7756e-17 after 50 (the "general" case; every other case is
    identical).  The test asserts four times the measured figure, and 4 * 2**-52 where that figure is zero (Q_BOUND): 8.8818e-16
    after one step, 1.1102e-16 after 50, both far inside 1e-13.  omega = 0 leaves q bit-identical.
  * the refusals of BodyPoses and of every invalid-argument branch of the four settings validators: codes and texts as the parent
    commit's nrs_ctx_impl.h states them (written out below, not read from the code under test), and a refused call changes nothing.
  * moving() / displaced() before and after set_pose, set_velocity, a rebuild and clear.
  * the same program once more under -fsanitize=address,undefined (a host program of its own: nothing is preloaded).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import bodies_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "nereus_amd", "csrc")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
E_INVALID = -1
Q_MEASURED = {1: 0.0, 50: 2.7756e-17}  # steps: largest |dq| measured (docstring)
Q_BOUND = {k: min(4.0 * v if v else 4.0 * 2.0 ** -52, 1e-13) for k, v in Q_MEASURED.items()}
DT = 1e-3


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_parts_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_parts") / "host_parts"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_parts_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_parts"), SANITIZE)


def hx(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


def cmd(name, *vals):
    """a command line: the name and the numbers of vals (scalars or sequences), flattened"""
    return name + "".join(" " + hx(x) for v in vals for x in np.ravel(np.asarray(v, np.float64)))


def run(exe, lines):
    """the program's answers, one per line, as (word, rest) pairs"""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [tuple((ln.split(" ", 1) + [""])[:2]) for ln in r.stdout.splitlines()]


def floats(rest):
    return np.array([float.fromhex(t) for t in rest.split()], np.float64)


def refusal(ans):
    word, rest = ans
    assert word == "rc"
    code, _, msg = rest.partition(" ")
    return int(code), msg


# ---- the cases of the pose integration -----------------------------------------------------------------------------------------
C0 = (0.4, 0.25, 0.125)
QN = (0.9, -0.3, 0.2, 0.5)  # not of unit length: set_pose normalises
CASES = {
    "translation": dict(v=(1.5, -0.2, 0.1), w=(0.0, 0.0, 0.0)),
    "spin_one_axis": dict(v=(0.0, 0.0, 0.0), w=(0.0, 0.0, 30.0)),
    "general": dict(v=(0.3, -0.2, 0.1), w=(4.0, -9.0, 30.0)),
    "tiny_angle": dict(v=(0.0, 0.0, 0.0), w=(1e-12 / DT, 0.0, 0.0)),
    "start_pose": dict(v=(0.5, 0.3, 0.0), w=(-7.0, 2.0, 11.0), x=(1.0, -2.0, 0.5), q=QN),
}


def case_lines(c, steps):
    lines = [cmd("init", 2, (0.0, 0.0, 0.0), C0)]
    if "q" in c:
        lines.append(cmd("pose", 1, c["x"], c["q"]))
    lines += [cmd("vel", 1, c["v"], c["w"]), cmd("adv", DT, steps), cmd("get", 1), cmd("rot", 1)]
    return lines


def model(c, steps):
    x, q = np.array(C0, np.float64), np.array([1.0, 0.0, 0.0, 0.0])
    if "q" in c:
        qq = np.array(c["q"], np.float64)
        x, q = np.array(c["x"], np.float64), qq / np.sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3])
    for _ in range(steps):
        x, q = bm.advance(x, q, c["v"], c["w"], DT)
    return x, q


def check_poses(exe):
    worst = {1: 0.0, 50: 0.0}
    for steps in (1, 50):
        for name, c in CASES.items():
            ans = run(exe, case_lines(c, steps))
            assert [a[0] for a in ans] == ["rc"] * (len(ans) - 2) + ["pose", "rot"] and all(refusal(a)[0] == 0 for a in ans[:-2]), (name, ans)
            got = floats(ans[-2][1])
            x, q = model(c, steps)
            dx = np.abs(got[:3] - x)
            dq = float(np.abs(got[3:] - q).max())
            print("%s, %d steps: max |dx| / ulp %.3g, max |dq| %.4e" % (name, steps, float((dx / np.spacing(np.abs(x))).max()), dq))
            assert np.all(dx <= steps * np.spacing(np.abs(x))), (name, steps, dx)
            if not np.any(c["w"]):
                assert np.array_equal(got[3:], q), (name, steps)  # omega = 0: q untouched
            worst[steps] = max(worst[steps], dq)
            assert dq <= Q_BOUND[steps], (name, steps, dq)
            assert abs(float(np.sqrt(got[3:] @ got[3:])) - 1.0) <= 4 * 2.0 ** -52
            # the rotation matrix the context rounds into the kernels' table: the model's, of the program's own q
            np.testing.assert_allclose(floats(ans[-1][1]).reshape(3, 3), bm.rotation(got[3:]), rtol=0, atol=4 * 2.0 ** -52)
    print("largest q difference: %r" % worst)


def test_pose_integration_matches_model(plain):
    check_poses(plain)


# ---- refusals: codes and texts of the parent commit ------------------------------------------------------------------------------
V0, W0, X0, Q0 = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0)
NO_BODIES = "the context has no boundary bodies (nrs_set_boundary_bodies first)"
BODY_REFUSALS = [
    # (commands before, the refused command, text)
    ([], cmd("vel", 1, V0, W0), NO_BODIES),
    ([], cmd("pose", 1, X0, Q0), NO_BODIES),
    ([], cmd("get", 1), NO_BODIES),
    (["I"], cmd("vel", 0, V0, W0), "body 0 is the static world"),
    (["I"], cmd("pose", 0, X0, Q0), "body 0 is the static world"),
    (["I"], cmd("get", 0), "body 0 is the static world"),
    (["I"], cmd("vel", 3, V0, W0), "unknown body"),
    (["I"], cmd("pose", 7, X0, Q0), "unknown body"),
    (["I"], cmd("get", 3), "unknown body"),
    (["I"], cmd("vel", 1, (np.nan, 0, 0), W0), "body velocity must be finite"),
    (["I"], cmd("vel", 1, V0, (0, np.inf, 0)), "body velocity must be finite"),
    (["I"], cmd("vel", 1, V0, (0, 0, -np.inf)), "body velocity must be finite"),
    (["I"], cmd("pose", 1, (0, np.nan, 0), Q0), "body pose must be finite"),
    (["I"], cmd("pose", 1, (np.inf, 0, 0), Q0), "body pose must be finite"),
    (["I"], cmd("pose", 1, X0, (1, np.nan, 0, 0)), "body pose must be finite"),
    (["I"], cmd("pose", 1, X0, (np.inf, 0, 0, 0)), "body pose must be finite"),
    (["I"], cmd("pose", 1, X0, (0, 0, 0, 0)), "zero quaternion"),
]
INIT3 = cmd("init", 3, (0, 0, 0), C0, (2.0, 2.0, 2.0))  # bodies 0, 1, 2
SETTINGS_REFUSALS = [
    # (command, text, the defaults the refused call must leave)
    (cmd("pci", 0.0, 3, 0, 0), "max_density_error must be > 0", "pci"),
    (cmd("pci", -1.0, 3, 0, 0), "max_density_error must be > 0", "pci"),
    (cmd("pci", np.nan, 3, 0, 0), "max_density_error must be > 0", "pci"),
    (cmd("pci", np.inf, 3, 0, 0), "max_density_error must be > 0", "pci"),
    (cmd("pci", 0.02, 0, 0, 0), "min_iters must be >= 1", "pci"),
    (cmd("pci", 0.02, 3, -0.1, 0), "prototype_spacing must be >= 0 (0 = cbrt(m / rho0))", "pci"),
    (cmd("pci", 0.02, 3, np.nan, 0), "prototype_spacing must be >= 0 (0 = cbrt(m / rho0))", "pci"),
    (cmd("pci", 0.02, 3, np.inf, 0), "prototype_spacing must be >= 0 (0 = cbrt(m / rho0))", "pci"),
    (cmd("pci", 0.02, 3, 0, -1.0), "delta must be >= 0 (0 = from the prototype)", "pci"),
    (cmd("pci", 0.02, 3, 0, np.nan), "delta must be >= 0 (0 = from the prototype)", "pci"),
    (cmd("pci", 0.02, 3, 0, np.inf), "delta must be >= 0 (0 = from the prototype)", "pci"),
    (cmd("pbf", -0.5, 2, 0.01, 0), "max_density_error must be >= 0 (0 = a fixed min_iters iterations)", "pbf"),
    (cmd("pbf", np.nan, 2, 0.01, 0), "max_density_error must be >= 0 (0 = a fixed min_iters iterations)", "pbf"),
    (cmd("pbf", np.inf, 2, 0.01, 0), "max_density_error must be >= 0 (0 = a fixed min_iters iterations)", "pbf"),
    (cmd("pbf", 0.02, 0, 0.01, 0), "min_iters must be >= 1", "pbf"),
    (cmd("pbf", 0.02, 2, 0.0, 0), "relaxation must be > 0", "pbf"),
    (cmd("pbf", 0.02, 2, np.nan, 0), "relaxation must be > 0", "pbf"),
    (cmd("pbf", 0.02, 2, np.inf, 0), "relaxation must be > 0", "pbf"),
    (cmd("pbf", 0.02, 2, 0.01, -0.1), "xsph must be in [0, 1]", "pbf"),
    (cmd("pbf", 0.02, 2, 0.01, 1.5), "xsph must be in [0, 1]", "pbf"),
    (cmd("pbf", 0.02, 2, 0.01, np.nan), "xsph must be in [0, 1]", "pbf"),
    (cmd("tens", -1.0, 0.2), "tensile k must be finite and >= 0 (0 = off)", "tens"),
    (cmd("tens", np.nan, 0.2), "tensile k must be finite and >= 0 (0 = off)", "tens"),
    (cmd("tens", np.inf, 0.2), "tensile k must be finite and >= 0 (0 = off)", "tens"),
    (cmd("tens", 0.1, 0.0), "tensile dq must be in (0, 1)", "tens"),
    (cmd("tens", 0.1, 1.0), "tensile dq must be in (0, 1)", "tens"),
    (cmd("tens", 0.1, np.nan), "tensile dq must be in (0, 1)", "tens"),
    (cmd("vort", -1.0), "vorticity eps_v must be finite and >= 0 (0 = off)", "vort"),
    (cmd("vort", np.nan), "vorticity eps_v must be finite and >= 0 (0 = off)", "vort"),
    (cmd("vort", np.inf), "vorticity eps_v must be finite and >= 0 (0 = off)", "vort"),
    (cmd("df", -1.0, 2, 1e-3, 1, 1), "DFSPH: max_density_error and max_divergence_error must be finite and >= 0", "df"),
    (cmd("df", np.nan, 2, 1e-3, 1, 1), "DFSPH: max_density_error and max_divergence_error must be finite and >= 0", "df"),
    (cmd("df", 1e-3, 2, -1.0, 1, 1), "DFSPH: max_density_error and max_divergence_error must be finite and >= 0", "df"),
    (cmd("df", 1e-3, 2, np.inf, 1, 1), "DFSPH: max_density_error and max_divergence_error must be finite and >= 0", "df"),
    (cmd("df", 1e-3, 0, 1e-3, 1, 1), "DFSPH: min_iters must be >= 1", "df"),
    (cmd("df", 1e-3, 2, 1e-3, 1, 2), "DFSPH: warm_start must be 0 or 1", "df"),
    (cmd("df", 1e-3, 2, 1e-3, 1, -1), "DFSPH: warm_start must be 0 or 1", "df"),
    (cmd("ak", -1.0, 0.0), "Akinci gamma must be finite and >= 0 (0 = off)", "ak"),
    (cmd("ak", np.nan, 0.0), "Akinci gamma must be finite and >= 0 (0 = off)", "ak"),
    (cmd("ak", np.inf, 0.0), "Akinci gamma must be finite and >= 0 (0 = off)", "ak"),
    (cmd("ak", 0.0, -1.0), "Akinci beta_adhesion must be finite and >= 0 (0 = off)", "ak"),
    (cmd("ak", 0.0, np.nan), "Akinci beta_adhesion must be finite and >= 0 (0 = off)", "ak"),
    (cmd("ak", 0.0, np.inf), "Akinci beta_adhesion must be finite and >= 0 (0 = off)", "ak"),
]
# the defaults of the parent commit's context members, as the program prints them
DEFAULTS = {"pci": [0.01, 3, 0.0, 0.0], "pbf": [0.01, 2, 0.01, 0.0], "tens": [0.0, 0.2], "vort": [0.0], "df": [1e-3, 2, 1e-3, 1, 1],
            "ak": [0.0, 0.0]}


def values(rest):
    return [float.fromhex(t) if "x" in t else float(int(t)) for t in rest.split()]


def check_refusals(exe):
    for before, line, text in BODY_REFUSALS:
        pre = [INIT3 if b == "I" else b for b in before]
        ans = run(exe, pre + [line, "state"] + ([cmd("get", 1)] if pre else []))
        assert refusal(ans[len(pre)]) == (E_INVALID, text), (line, ans)
        # a refused call changes nothing: not moving, not displaced, not dirty, the pose still the centroid
        assert ans[len(pre) + 1] == ("state", "%d 0 0 0 0" % (3 if pre else 0)), (line, ans)
        if pre:
            assert np.array_equal(floats(ans[-1][1]), np.array(C0 + (1.0, 0.0, 0.0, 0.0))), (line, ans)
    for line, text, kind in SETTINGS_REFUSALS:
        ans = run(exe, [line])
        assert refusal(ans[0]) == (E_INVALID, text), (line, ans)
        assert ans[1][0] == kind and values(ans[1][1]) == [float(v) for v in DEFAULTS[kind]], (line, ans)


def test_refusals_keep_codes_and_texts(plain):
    check_refusals(plain)


def check_settings_accepted(exe):
    lines = [cmd("pci", 0.02, 5, 0.01, 2.5), cmd("pbf", 0.0, 4, 0.5, 1.0), cmd("tens", 0.1, 0.3), cmd("tens", 0.0, 0.5), cmd("vort", 0.25),
             cmd("df", 0.0, 3, 0.0, 0, 0), cmd("ak", 0.7, 0.0), cmd("ak", 0.0, 1.25), cmd("pbf", 0.02, 2, 0.01, 1.5)]
    ans = run(exe, lines)
    want = [[0.02, 5, 0.01, 2.5], [0.0, 4, 0.5, 1.0], [0.1, 0.3], [0.0, 0.5], [0.25], [0.0, 3, 0.0, 0, 0], [0.7, 0.0], [0.0, 1.25]]
    for i, w in enumerate(want):
        assert refusal(ans[2 * i])[0] == 0 and values(ans[2 * i + 1][1]) == [float(v) for v in w], (lines[i], ans[2 * i:2 * i + 2])
    # a refused call after an accepted one keeps the accepted values
    assert refusal(ans[-2]) == (E_INVALID, "xsph must be in [0, 1]") and values(ans[-1][1]) == [0.0, 4.0, 0.5, 1.0]


def test_settings_accepted(plain):
    check_settings_accepted(plain)


# ---- moving() / displaced() ------------------------------------------------------------------------------------------------------
def check_moving_displaced(exe):
    qn = np.array(QN) / np.sqrt(np.dot(QN, QN))
    script = [
        ("state", "0 0 0 0 0"),                                 # no assignment
        (INIT3, None), ("state", "3 0 0 0 0"),                  # assigned, at rest
        (cmd("pose", 1, X0, QN), None), ("state", "3 1 1 1 0"),  # a pose was set: dirty until the tables are rebuilt, and displaced
        ("rebuilt", None), ("state", "3 0 1 0 0"),              # rebuilt: displaced, no longer moving
        (cmd("vel", 1, (0, 0, 0), (0, 0, 2.0)), None), ("state", "3 1 1 0 1"),  # a velocity: moving
        (cmd("vel", 1, V0, W0), None), ("state", "3 0 1 0 0"),
        (cmd("pose", 1, C0, (2.0, 0, 0, 0)), None), ("state", "3 1 0 1 0"),  # back at the rest pose (2 normalises to 1): dirty, not displaced
        ("rebuilt", None), ("state", "3 0 0 0 0"),
        (cmd("vel", 2, (1.0, 0, 0), W0), None), ("state", "3 1 0 0 0"),      # body 2 moves: moving; displaced only once it is advanced
        (cmd("adv", DT, 1), None), ("state", "3 1 1 0 0"),
        (cmd("pose", 1, X0, QN), None), ("clear", None), ("state", "0 0 0 0 0"),  # clear drops assignment and dirt
        (INIT3, None), ("state", "3 0 0 0 0"),                  # a new assignment starts at rest
    ]
    ans = run(exe, [s[0] for s in script])
    for (line, want), a in zip(script, ans):
        if want is None:
            assert refusal(a)[0] == 0, (line, a)
        else:
            assert a == ("state", want), (line, a)
    # the pose set_pose stored is the normalised one
    got = floats(run(exe, [INIT3, cmd("pose", 1, X0, QN), cmd("get", 1)])[-1][1])
    assert np.array_equal(got[:3], np.array(X0)) and np.abs(got[3:] - qn).max() <= 2.0 ** -52


def test_moving_and_displaced(plain):
    check_moving_displaced(plain)


def test_under_sanitizers(sanitized):
    check_poses(sanitized)
    check_refusals(sanitized)
    check_settings_accepted(sanitized)
    check_moving_displaced(sanitized)
