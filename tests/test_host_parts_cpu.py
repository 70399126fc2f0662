"""The library's HIP-free host components (nereus_amd/csrc/nrs_host_bodies.h, nrs_host_settings.h, nrs_host_slab.h) without a GPU: a stand-alone
program (tests/host_parts_main.cpp) built with the host compiler, -ffp-contract=off as the library is, fed commands on stdin.

  * the pose integration against tests/bodies_model.advance, for 1 and for 50 consecutive steps.  x: 1 ulp per component per step
    (the same two IEEE operations on both sides; measured: identical).  q: the largest component difference these cases give,
    measured where this test was written, is 0 after one step and 2.7756e-17 after 50 (the "general" case; every other case is
    identical).  The test asserts four times the measured figure, and 4 * 2**-52 where that figure is zero (Q_BOUND): 8.8818e-16
    after one step, 1.1102e-16 after 50, both far inside 1e-13.  omega = 0 leaves q bit-identical.
  * the refusals of BodyPoses and of every invalid-argument branch of the four settings validators: codes and texts as the parent
    commit's nrs_ctx_impl.h states them (written out below, not read from the code under test), and a refused call changes nothing.
  * moving() / displaced() before and after set_pose, set_velocity, a rebuild and clear.
  * the host decisions of the slab exchange (nrs_host_slab.h): the cell-table window, the full truth table of the partition form,
    the refusals of nrs_slab_configure in their order of precedence, what finish() makes of a pack's stream totals (consistency,
    overflow after storing) and the arithmetic of the unpack (header and capacity refusals at the limit and one over, piece offsets,
    n and n_owned).  The expectations restate the rule of the commit before the header existed (its nrs_ctx_impl.h: choose_window,
    slab_configure, slab_pack, finish_pack, slab_unpack); nothing is read from the code under test.
  * the grid nrs_set_boundaries makes from the boundary particles' bounding box (nrs_host_grid.h), in both precisions, hex-float
    exact against the rule of the commit before the header existed (its nrs_ctx_impl.h, set_boundaries) restated here: a single
    point, extents that are whole multiples of h and one ulp to either side, extents whose cell count lands on a power of two and
    just over it, negative coordinates, exactly 2^31 cells (accepted) and 2^32 (refused, with the text, and nothing written).
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
E_INVALID, E_HIP, E_CAPACITY = -1, -2, -3
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


# ---- the slab exchange's host decisions (nrs_host_slab.h) ------------------------------------------------------------------------
def ints(ans, word):
    assert ans[0] == word, ans
    return [int(t) for t in ans[1].split()]


def check_slab_window(exe):
    g = (256, 64, 64)
    # the slab [100, 120) with halo 2 and two columns of drift is [96, 124); 8 columns of slack either side: [88, 132), 44 columns,
    # rounded up to 64.  [100, 128) still fits [88, 152).  [56, 204) does not, and with its slack needs 256 columns: the whole grid.
    ans = run(exe, [cmd("win", g, 100, 120, 2, 0), cmd("win", g, 104, 124, 2, 0), cmd("win", g, 60, 200, 2, 0), cmd("win", g, 60, 200, 2, 0)])
    assert [ints(a, "win") for a in ans] == [[1, 88, 64], [0, 88, 64], [1, 0, 0], [0, 0, 0]]
    # a grid with an axis that is no power of two has no window; "changed" only if there was one
    for bad in ((256, 48, 64), (256, 64, 96), (192, 64, 64)):
        ans = run(exe, [cmd("win", bad, 100, 120, 2, 0), cmd("win", g, 100, 120, 2, 0), cmd("win", bad, 100, 120, 2, 0), cmd("win", bad, 100, 120, 2, 1)])
        assert [ints(a, "win") for a in ans] == [[0, 0, 0], [1, 88, 64], [1, 0, 0], [0, 0, 0]], bad
    # force chooses afresh although the old window fits: [100, 128) with slack is [92, 136)
    ans = run(exe, [cmd("win", g, 100, 120, 2, 0), cmd("win", g, 104, 124, 2, 1), cmd("win", g, 104, 124, 2, 1)])
    assert [ints(a, "win") for a in ans] == [[1, 88, 64], [1, 92, 64], [0, 92, 64]]
    # clipped at both ends of the grid ([236, 256) with slack starts at 228); an empty range (the slab lies outside the grid) has no window
    ans = run(exe, [cmd("win", g, 0, 20, 2, 0), cmd("win", g, 240, 256, 2, 0), cmd("win", g, 300, 320, 2, 0), cmd("win", g, -50, -20, 2, 0)])
    assert [ints(a, "win") for a in ans] == [[1, 0, 32], [1, 228, 32], [1, 0, 0], [0, 0, 0]]


RESORT_MIN = 32768  # nrs_kernels_resort.h


def form_model(cv, so, rb, hc, hn, hd, cn, n):
    """slab_pack's conditions before the header existed: (form, counts cell changers)"""
    if n == 0:
        return 0, 0
    if cv and so and cn == n and rb and hc and hn and hd:
        return 2, 1
    resort = rb and so and hc and hn and hd
    return (1 if resort and n >= RESORT_MIN else 0), int(bool(resort))


def check_slab_form(exe):
    cases = []
    for m in range(64):
        b = [(m >> k) & 1 for k in range(6)]
        for n in (0, 1, RESORT_MIN - 1, RESORT_MIN, 100000):
            for cn in (n, n + 1, 0):
                cases.append(b + [cn, n])
    ans = run(exe, [cmd("form", c, RESORT_MIN) for c in cases])
    seen = set()
    for c, a in zip(cases, ans):
        want = form_model(*c)
        assert tuple(ints(a, "form")) == want, (c, a)
        seen.add((want, c[7] >= RESORT_MIN))
    # every outcome occurs, among them: compacting with cell changers counted one particle below the threshold, in place at it, and
    # pre-classified below it (the form does not look at the threshold: the step that classifies does)
    assert seen >= {((0, 0), False), ((0, 0), True), ((0, 1), False), ((1, 1), True), ((2, 1), False), ((2, 1), True)}
    all_true = [1, 1, 1, 1, 1, 1]
    one = lambda c: tuple(ints(run(exe, [cmd("form", c, RESORT_MIN)])[0], "form"))
    assert one(all_true + [RESORT_MIN - 1, RESORT_MIN - 1]) == (2, 1)
    assert one(all_true + [RESORT_MIN, RESORT_MIN - 1]) == (0, 1) and one(all_true + [RESORT_MIN - 1, RESORT_MIN]) == (1, 1)  # classifiedN != N
    assert one([1, 1, 1, 1, 1, 0, RESORT_MIN, RESORT_MIN]) == (0, 0)   # hashNext == hashCur
    assert one(all_true + [0, 0]) == (0, 0)                            # N == 0


SESPH, IISPH, PCISPH, PBF, DFSPH = range(5)
T_BODIES = "contexts with boundary bodies have no slab decomposition"
T_IISPH = "IISPH slabs need a halo of at least 8 cells (2 * iterations + 4)"
T_HALO = "halo must be >= 2 cells (one cell for the density of the ring + one)"
T_NARROW = "slab narrower than two halos"
CONFIGURE = [
    # (solver, has bodies, lo, hi, halo, refusal text or None), in the order of precedence: every line is also wrong in all later ways
    (SESPH, 1, 5, 6, 1, T_BODIES), (IISPH, 1, 5, 6, 1, T_BODIES), (PCISPH, 1, 5, 6, 1, T_BODIES), (PBF, 1, 5, 6, 1, T_BODIES),
    (DFSPH, 1, 5, 6, 1, T_BODIES), (SESPH, 1, 0, 100, 2, T_BODIES),
    (PCISPH, 0, 5, 6, 1, "PCISPH contexts have no slab decomposition"), (PCISPH, 0, 0, 100, 8, "PCISPH contexts have no slab decomposition"),
    (PBF, 0, 5, 6, 1, "PBF contexts have no slab decomposition"), (PBF, 0, 0, 100, 8, "PBF contexts have no slab decomposition"),
    (DFSPH, 0, 5, 6, 1, "DFSPH contexts have no slab decomposition"), (DFSPH, 0, 0, 100, 8, "DFSPH contexts have no slab decomposition"),
    (IISPH, 0, 5, 6, 1, T_IISPH), (IISPH, 0, 0, 100, 7, T_IISPH), (IISPH, 0, 0, 100, -3, T_IISPH),
    (SESPH, 0, 5, 6, 1, T_HALO), (SESPH, 0, 0, 100, 1, T_HALO), (SESPH, 0, 0, 100, 0, T_HALO), (SESPH, 0, 0, 100, -1, T_HALO),
    (SESPH, 0, 5, 8, 2, T_NARROW), (SESPH, 0, 8, 5, 2, T_NARROW), (IISPH, 0, 0, 15, 8, T_NARROW), (SESPH, 0, -2 ** 31, -2 ** 31 + 3, 2, T_NARROW),
    (SESPH, 0, 5, 9, 2, None), (IISPH, 0, 0, 16, 8, None), (SESPH, 0, -2 ** 31, 2 ** 31 - 1, 2, None), (SESPH, 0, -3, 1, 2, None),
]


def check_slab_configure(exe):
    ans = run(exe, [cmd("cfg", *c[:5]) for c in CONFIGURE])
    for c, a in zip(CONFIGURE, ans):
        assert refusal(a) == ((0, "") if c[5] is None else (E_INVALID, c[5])), (c, a)


COMPACT, INPLACE, PRECLASSIFIED = 0, 1, 2
T_TOTALS, T_OVERFLOW = "inconsistent slab stream totals", "slab message capacity exceeded"


def finish(exe, form, n, mcap, raw, scan=(0, 0), before=()):
    """the answers to one queue + fin: (code, text), [stored, n, form, movers, pending], the seven stored totals"""
    ans = run(exe, list(before) + [cmd("queue", form, 1, n, mcap), cmd("fin", raw, scan)])[-3:]
    assert refusal(ans[0])[0] == 0
    v = ints(ans[2], "fin")
    return refusal(ans[1]), v[:5], v[5:]


def check_slab_finish(exe):
    # totals: stay, migrants / halo copies to the left, to the right, ghosts, cell changers
    raw = [90, 4, 6, 5, 7, 8, 30]
    for form in (COMPACT, INPLACE):
        assert finish(exe, form, 100, 12, raw) == ((0, ""), [1, 90, form, 30, 0], raw)
    # pre-classified: the cell changers and the stay count (N - dead) come from the re-sort's scan, whatever k_slab_scan's say
    assert finish(exe, PRECLASSIFIED, 100, 12, [1, 4, 6, 5, 7, 8, 99], scan=(30, 10)) == ((0, ""), [1, 90, PRECLASSIFIED, 30, 0], raw)
    # ... and in the other forms the scan's figures are not looked at
    assert finish(exe, INPLACE, 100, 12, raw, scan=(55, 66)) == ((0, ""), [1, 90, INPLACE, 30, 0], raw)
    # N == 0: the landing is not read (nothing was copied there)
    assert finish(exe, COMPACT, 0, 12, raw) == ((0, ""), [1, 0, COMPACT, 0, 0], [0] * 7)
    # inconsistent totals: nothing is stored (the totals of the pack before stay), the pack is no longer pending
    first = [cmd("queue", COMPACT, 0, 50, 12), cmd("fin", [40, 1, 1, 1, 1, 1, 3], (0, 0))]
    for form, n, bad, scan in ((COMPACT, 100, [92, 4, 6, 5, 7, 8, 30], (0, 0)),     # stay + migrants = 101 > N
                               (INPLACE, 100, [90, 4, 6, 5, 7, 8, 91], (0, 0)),     # more cell changers than stayers
                               (PRECLASSIFIED, 100, raw, (91, 10)),                 # the same from the scan
                               (PRECLASSIFIED, 100, raw, (30, 0)),                  # no dead slot, yet 9 migrants
                               (PRECLASSIFIED, 100, raw, (30, 101))):               # more dead slots than slots (N - dead wraps)
        assert finish(exe, form, n, 12, bad, scan, before=first) == ((E_HIP, T_TOTALS), [0, 0, 0, 0, 0], [40, 1, 1, 1, 1, 1, 3]), (form, bad, scan)
    assert finish(exe, COMPACT, 100, 12, [91, 4, 6, 5, 7, 8, 91])[0] == (0, "")     # at both limits
    # each overflow condition at the limit and one over; the counts are stored either way
    for form in (COMPACT, INPLACE, PRECLASSIFIED):
        scan = (30, 10)
        for t in ([90, 4, 8, 5, 7, 8, 30], [90, 4, 6, 5, 7, 12, 30], [90, 3, 9, 6, 6, 12, 30]):   # left, right + ghosts, all three at 12
            assert finish(exe, form, 100, 12, t, scan) == ((0, ""), [1, 90, form, 30, 0], t)
        for t in ([90, 4, 9, 5, 7, 8, 30], [90, 4, 6, 5, 8, 8, 30], [90, 4, 6, 5, 7, 13, 30]):     # left, right, ghosts at 13
            assert finish(exe, form, 100, 12, t, scan) == ((E_CAPACITY, T_OVERFLOW), [1, 90, form, 30, 0], t)


T_HEADER, T_CONTEXT = "corrupt slab message header", "owned + halo particles exceed the context capacity"


def unpack(exe, form, ghosts, left, right, n, phys, holes, mcap, cap):
    """queue + fin (a pack of n + 10 particles, of which n stay and `ghosts` are ghosts) and the unpack"""
    before = [cmd("queue", form, 0, n + 10, 1000), cmd("fin", [n, 0, 0, 0, 0, ghosts, 0], (0, 10))]
    hdr = lambda h: (0, 0, 0) if h is None else (1,) + tuple(h)
    ans = run(exe, before + [cmd("unp", hdr(left), hdr(right), n, phys, holes, mcap, cap)])[3:]
    return refusal(ans[0]), (ints(ans[1], "unp") if len(ans) > 1 else None)


def check_slab_unpack(exe):
    # hand-written: 92 owned, 5 ghosts, 3 migrants + 4 halo copies from the left, 2 + 6 from the right.  Pieces in the order
    # migrants left, migrants right, ghosts, halo left, halo right: offsets 0, 3, 5, 10, 14, 20.
    start = [0, 3, 5, 10, 14, 20]
    # compacting form: appended behind the n owned particles
    assert unpack(exe, COMPACT, 5, (3, 4), (2, 6), 92, 0, 0, 10, 112) == ((0, ""), [0] + start + [92, 20, 112, 97])
    # in place with the holes still there: appended behind the physical extent
    for form in (INPLACE, PRECLASSIFIED):
        assert unpack(exe, form, 5, (3, 4), (2, 6), 92, 102, 1, 10, 122) == ((0, ""), [1] + start + [102, 20, 112, 97])
        # ... and once something has compacted the holes (a download between pack and unpack), behind the n live ones
        assert unpack(exe, form, 5, (3, 4), (2, 6), 92, 102, 0, 10, 112) == ((0, ""), [0] + start + [92, 20, 112, 97])
    # a missing left / right / both messages: its pieces are empty, whatever the bytes would have said
    assert unpack(exe, COMPACT, 5, None, (2, 6), 92, 0, 0, 10, 200) == ((0, ""), [0, 0, 0, 2, 7, 7, 13, 92, 13, 105, 94])
    assert unpack(exe, COMPACT, 5, (3, 4), None, 92, 0, 0, 10, 200) == ((0, ""), [0, 0, 3, 3, 8, 12, 12, 92, 12, 104, 95])
    assert unpack(exe, INPLACE, 5, None, None, 92, 102, 1, 10, 200) == ((0, ""), [1, 0, 0, 0, 5, 5, 5, 102, 5, 97, 92])
    # header sums at the message capacity and one over, on either side; the header is checked before the capacity
    assert unpack(exe, COMPACT, 5, (3, 7), (4, 6), 92, 0, 0, 10, 200)[0] == (0, "")
    assert unpack(exe, COMPACT, 5, (4, 7), (4, 6), 92, 0, 0, 10, 200) == ((E_INVALID, T_HEADER), None)
    assert unpack(exe, COMPACT, 5, (3, 7), (10, 1), 92, 0, 0, 10, 200) == ((E_INVALID, T_HEADER), None)
    assert unpack(exe, COMPACT, 5, (2 ** 32 - 1, 1), None, 92, 0, 0, 10, 200) == ((E_INVALID, T_HEADER), None)   # (no 32-bit wrap)
    assert unpack(exe, COMPACT, 5, (4, 7), (4, 6), 92, 0, 0, 10, 5) == ((E_INVALID, T_HEADER), None)
    # base + arrivals at the context capacity and one over, in both placements
    assert unpack(exe, COMPACT, 5, (3, 4), (2, 6), 92, 0, 0, 10, 111) == ((E_CAPACITY, T_CONTEXT), None)
    assert unpack(exe, INPLACE, 5, (3, 4), (2, 6), 92, 102, 1, 10, 122)[0] == (0, "")
    assert unpack(exe, INPLACE, 5, (3, 4), (2, 6), 92, 102, 1, 10, 121) == ((E_CAPACITY, T_CONTEXT), None)


# ---- the grid from the boundary AABB (nrs_host_grid.h) ----------------------------------------------------------------------------
T_GRID = "grid from boundary AABB exceeds 2^31 cells"


def grid_model(real, pts, h):
    """set_boundaries of the commit before: SReal min / max, origin = (SReal)(min - 0.1), extent = next_pow2((uint32)ceil((max - min
    + 0.1) / h)) with max - min in SReal and the rest in double; None beyond 2^31 cells"""
    pts = np.asarray(pts, real).reshape(-1, 3)
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    origin = (mn.astype(np.float64) - 0.1).astype(real)
    size = []
    for a in range(3):
        sz = int(np.ceil((np.float64(real(mx[a] - mn[a])) + 0.1) / np.float64(real(h))))
        v = (sz - 1) & 0xFFFFFFFF
        for k in (1, 2, 4, 8, 16):
            v |= v >> k
        size.append((v + 1) & 0xFFFFFFFF)
    cells = size[0] * size[1] * size[2]
    return None if cells > 2 ** 31 else (origin, size, cells)


def straddle(real, k, h):
    """the two neighbouring SReal extents e0 < e1 with ceil((e0 + 0.1) / h) = k and ceil((e1 + 0.1) / h) = k + 1"""
    q = lambda e: int(np.ceil((np.float64(e) + 0.1) / np.float64(real(h))))
    e = real(k * np.float64(real(h)) - 0.1)
    while q(e) > k:
        e = np.nextafter(e, real(-np.inf))
    while q(np.nextafter(e, real(np.inf))) <= k:
        e = np.nextafter(e, real(np.inf))
    return e, np.nextafter(e, real(np.inf))


def grid_cases(real):
    h = 0.0457
    up, dn = (lambda v: np.nextafter(real(v), real(np.inf))), (lambda v: np.nextafter(real(v), real(-np.inf)))
    cases = [(h, [(1.0, 2.0, 3.0)]),                                               # a single point: ceil(0.1 / h) = 3 -> 4 cells
             (h, [(-3.25, -0.5, -7.0), (-1.0, -0.25, -6.5), (-2.0, -0.4, -6.75)]),  # negative coordinates, min and max in different points
             (0.125, [(0.0, 0.0, 0.0), (1.0, 2.0, 4.0)])]                          # extents 8 h, 16 h, 32 h exactly: (e + 0.1) / h = 8.8, 16.8, 32.8
    cases += [(0.125, [(0.0, 0.0, 0.0), (f(1.0), f(2.0), f(4.0))]) for f in (up, dn)]  # ... and one ulp to either side
    for k in (16, 64):                                                             # ceil = 2^m: that many cells; one ulp more: twice as many
        e0, e1 = straddle(real, k, h)
        cases += [(h, [(0.5, -1.0, 0.0), (0.5 + 0.0, -1.0, e)]) for e in (e0, e1)]
        cases += [(h, [(0.0, 0.0, 0.0), (e, 1.0, 1.0)]) for e in (e0, e1)]
    cases += [(1.0, [(-700.0, 0.0, 0.0), (800.0, 900.0, 900.0)]),                  # 2048 x 1024 x 1024 = 2^31 cells: accepted
              (1.0, [(-700.0, 0.0, 0.0), (800.0, 1100.0, 900.0)]),                 # 2048 x 2048 x 1024 = 2^32: refused
              (0.0457, [(0.0, 0.0, 0.0), (5773.5, 5773.5, 5773.5)])]               # 2^17 cells on every axis: refused
    return cases


def check_grid(exe):
    for real, prec in ((np.float32, 32), (np.float64, 64)):
        cases = grid_cases(real)
        lines = [cmd("grid", prec, real(h), len(pts), np.asarray(pts, real)) for h, pts in cases]
        ans = run(exe, lines)
        seen = []
        for i, (h, pts) in enumerate(cases):
            want = grid_model(real, pts, h)
            got = ans[2 * i + 1][1].split()
            if want is None:
                assert refusal(ans[2 * i]) == (E_INVALID, T_GRID), (prec, pts, ans[2 * i])
                assert [float.fromhex(t) for t in got[:3]] == [7.0] * 3 and got[3:] == ["7"] * 4, (prec, pts, got)   # nothing was written
                seen.append(None)
                continue
            assert refusal(ans[2 * i]) == (0, ""), (prec, pts, ans[2 * i])
            origin, size, cells = want
            assert [float.fromhex(t) for t in got[:3]] == [float(v) for v in origin], (prec, h, pts, got, want)   # (exact: hex floats)
            assert got[3:] == [str(v) for v in size] + [str(cells)], (prec, h, pts, got, want)
            seen.append(size)
        # written out by hand: what the cases are there to show
        assert seen[0] == [4, 4, 4] and seen[2] == [16, 32, 64] and seen[3] == [16, 32, 64] and seen[4] == [16, 32, 64]
        assert [s[2] for s in seen[5:7]] == [16, 32] and [s[0] for s in seen[7:9]] == [16, 32]
        assert [s[2] for s in seen[9:11]] == [64, 128] and [s[0] for s in seen[11:13]] == [64, 128]
        assert seen[13] == [2048, 1024, 1024] and seen[14] is None and seen[15] is None
        first = floats(ans[1][1])[:3]
        assert np.array_equal(first, (np.asarray([1.0, 2.0, 3.0], real).astype(np.float64) - 0.1).astype(real).astype(np.float64))
    # the key width of the sorts: the bits of numCells - 1, at least 1
    cells = [1, 2, 3, 4, 5, 2 ** 24, 2 ** 24 + 1, 2 ** 27, 2 ** 31]
    ans = run(exe, [cmd("keybits", c) for c in cells])
    assert [ints(a, "keybits")[0] for a in ans] == [1, 1, 2, 2, 3, 24, 25, 27, 31]


def test_grid_from_boundary_box(plain):
    check_grid(plain)


def test_slab_window(plain):
    check_slab_window(plain)


def test_slab_form_truth_table(plain):
    check_slab_form(plain)


def test_slab_configure_refusals_in_order(plain):
    check_slab_configure(plain)


def test_slab_finish(plain):
    check_slab_finish(plain)


def test_slab_unpack_arithmetic(plain):
    check_slab_unpack(plain)


def test_under_sanitizers(sanitized):
    check_grid(sanitized)
    check_slab_window(sanitized)
    check_slab_form(sanitized)
    check_slab_configure(sanitized)
    check_slab_finish(sanitized)
    check_slab_unpack(sanitized)
    check_poses(sanitized)
    check_refusals(sanitized)
    check_settings_accepted(sanitized)
    check_moving_displaced(sanitized)
