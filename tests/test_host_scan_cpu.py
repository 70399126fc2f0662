"""The scan geometry the host prepares (nereus_amd/csrc/nrs_host_scan.h) without a GPU: the header itself, compiled with the host
compiler into a stand-alone program (tests/host_scan_main.cpp; -ffp-contract=off as the library is), fed commands on stdin.  Brute
force in numpy is the reference, never the code under test.

  * make_thresholds<R>, R = float and double: for every float within 64 ulps either side of each returned cut-off the cut-off
    decides exactly what the kernels' predicate decides — x < lenLtIr <=> (R)sqrtf(x) < ir, and x < r2LeH2 <=> not
    ((R)(sqrtf(x) * sqrtf(x)) > ir * ir), the product formed in float as length() * length() is — and lenLtIr <= r2LeH2.
  * scan_quant: qc.s, qc.o, qT and ok, hex-float and integer exact against the formula restated here in numpy float32 / float64, for
    cells of h, 1.3 h, 0.53 h and all three at once, in both precisions; each of the four refusals by one input that trips it alone;
    and qT equal to threshold() of tests/test_quantised_scan_model.py on that file's scenes, which ties the model to the code.
  * the superset guarantee on the library's quantiser and cut-offs: the scenes of test_quantised_scan_model.py, point for point (a
    file of float32), every pair, exact test dot(d, d) < r2LeH2 (the wider cut-off, the WIDE scan's), integer test d2 < qT: no exact
    hit is missed, no owner is out of the quantiser's range; and the model's bound on the false positives on its 3000-point scene.
  * window_params on a 64 x 32 x 32 grid: no window, a window as wide as the grid, a narrower one; only numBodies, gridSize[0] and
    numCells change.  is_pow2, pow2_grid, wall_blocks at their edges.
  * the same program once more under -fsanitize=address,undefined (a host program of its own: nothing is preloaded).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import test_quantised_scan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "nereus_amd", "csrc"),
         "-I", os.path.join(ROOT, "include")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
QP_PER_CELL, QP_MARGIN, QP_HALF = np.float32(256.0), np.float32(2.5), np.float32(511.0)
REAL = {32: np.float32, 64: np.float64}
H = 0.0457  # the scenes' interaction radius


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "host_scan_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_scan") / "host_scan"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_scan_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_scan"), SANITIZE)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """the model's scenes as files of float32: [(file, n, h, cs, origin, centre_cells, cs_over_h)], and the false-positive scene"""
    d = tmp_path_factory.mktemp("host_scan_scenes")
    out = []
    for cs_over_h in model.CS_OVER_H:
        for centre in model.CENTRES:
            h, cs, origin, pos = model.superset_scene(centre, cs_over_h)
            f = str(d / ("scene_%g_%g.f32" % (centre, cs_over_h)))
            pos.astype("<f4").tofile(f)
            out.append((f, len(pos), h, cs, origin, centre, cs_over_h))
    h, cs, origin, pos = model.false_positive_scene()
    f = str(d / "false_positives.f32")
    pos.astype("<f4").tofile(f)
    return out, (f, len(pos), h, cs, origin)


def hx(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


def run(exe, lines):
    """the program's answers, one per line, as lists of words behind the answer's name"""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    ans = [ln.split() for ln in r.stdout.splitlines()]
    assert len(ans) == len(lines), (len(ans), len(lines))
    return ans


# ---- the cut-offs ------------------------------------------------------------------------------------------------------------------
INEXACT = [1.0 / 3.0, 0.7, 1.1]  # as floats: full mantissas, the square is not a float
RADII = [H, 0.01, 0.1, 1.0, 3.7, 2.0 ** -10, 2.0 ** 3] + INEXACT


def threshold_radii():
    """(prec, ir) with ir of type R: every radius as a float in both precisions, and as the double that is no float"""
    out = []
    for v in RADII:
        f = np.float32(v)
        out += [(32, f), (64, np.float64(f))]
        if np.float64(f) != np.float64(v):
            out.append((64, np.float64(v)))
    for v in INEXACT:
        f = np.float64(np.float32(v))
        assert np.float64(np.float32(f * f)) != f * f
    assert sum(1 for p, ir in out if p == 64 and np.float64(np.float32(ir)) != ir) >= 7
    return out


def ulp_window(T, k=64):
    """the floats within k ulps either side of the positive float T"""
    bits = np.array([T], np.float32).view(np.int32)[0]
    assert bits - k > 0
    return (bits + np.arange(-k, k + 1, dtype=np.int32)).astype(np.int32).view(np.float32)


def check_thresholds(exe):
    cases = threshold_radii()
    ans = run(exe, ["thr %d %s" % (prec, hx(ir)) for prec, ir in cases])
    for (prec, ir), a in zip(cases, ans):
        real = REAL[prec]
        assert a[0] == "thr"
        lenLtIr, r2LeH2 = (float.fromhex(t) for t in a[1:])
        assert np.float32(lenLtIr) == lenLtIr and np.float32(r2LeH2) == r2LeH2 and 0 < lenLtIr <= r2LeH2, (prec, ir, a)
        x = np.unique(np.concatenate([ulp_window(np.float32(lenLtIr)), ulp_window(np.float32(r2LeH2))]))
        length = np.sqrt(x)                                      # sqrtf: correctly rounded float32
        assert length.dtype == np.float32
        inside = length.astype(real) < real(ir)                  # length(r) < ir
        r2 = (length * length).astype(real)                      # R r2 = length(r) * length(r): a float product, then SReal
        h2 = real(ir) * real(ir)
        assert r2.dtype == real and type(h2) is real
        not_beyond = ~(r2 > h2)                                  # !(r2 > h2)
        print("R%d ir %s: lenLtIr %s r2LeH2 %s (%d floats apart), %d floats checked" % (
            prec, hx(ir), hx(lenLtIr), hx(r2LeH2), int(np.float32(r2LeH2).view(np.int32)) - int(np.float32(lenLtIr).view(np.int32)), len(x)))
        assert np.array_equal(x < np.float32(lenLtIr), inside), (prec, ir, a)
        assert np.array_equal(x < np.float32(r2LeH2), not_beyond), (prec, ir, a)
        assert inside.any() and not inside.all() and not_beyond.any() and not not_beyond.all()


def test_thresholds_decide_as_the_kernels_predicates(plain):
    check_thresholds(plain)


# ---- the quantisation set-up ---------------------------------------------------------------------------------------------------------
def quant_formula(real, grid, origin, cs, ir):
    """scan_quant restated: (s[3], o[3], qT, ok) with float32 and float64 where the context uses float and double"""
    with np.errstate(all="ignore"):
        cs, origin, ir = np.asarray(cs, real), np.asarray(origin, real), real(ir)
        s = (QP_PER_CELL / cs.astype(np.float32)).astype(np.float32)
        r = (np.float32(ir) * s).astype(np.float32)
        ok = grid[0] >= 4
        for a in range(3):
            ok = ok and bool(cs[a] > 0) and bool(np.isfinite(s[a])) and bool(np.float32(r[a] + QP_MARGIN) < QP_HALF)
        hq = np.float32(max(np.float32(0.0), r[0], r[1], r[2]))
        lim = np.float64(hq) + np.float64(QP_MARGIN)
        qT = int(np.ceil(lim * lim)) + 1 if ok else 0
    return s, origin.astype(np.float64), qT, ok


def quant_line(prec, grid, origin, cs, ir):
    return "quant %d %d %d %d " % ((prec,) + tuple(grid)) + " ".join(hx(v) for v in list(origin) + list(cs) + [ir])


def quant_answer(a):
    assert a[0] == "quant"
    return [float.fromhex(t) for t in a[1:4]], [float.fromhex(t) for t in a[4:7]], int(a[7]), int(a[8])


def check_quant_setup(exe):
    for prec, real in REAL.items():
        h = real(np.float32(H)) if prec == 32 else real(H)
        origin = np.asarray([-1.1, 0.25, 3.0], real)
        cases = [((64, 32, 32), origin, [real(k * h)] * 3, h) for k in (1.0, 1.3, 0.53)]
        cases.append(((64, 32, 32), origin, [real(h), real(1.3 * h), real(0.53 * h)], h))   # the threshold follows the narrowest cell
        cases.append(((4, 2, 2), origin, [real(h)] * 3, h))                                  # four columns are enough; y and z are not looked at
        ans = run(exe, [quant_line(prec, *c) for c in cases])
        for c, a in zip(cases, ans):
            s, o, qT, ok = quant_answer(a)
            ws, wo, wqT, wok = quant_formula(real, *c)
            print("R%d cells %s: s %s qT %d ok %d" % (prec, [hx(v) for v in c[2]], [hx(v) for v in s], qT, ok))
            assert s == [float(v) for v in ws] and o == [float(v) for v in wo] and (qT, ok) == (wqT, int(wok)), (prec, c, a, (ws, wo, wqT, wok))
            assert ok == 1
        # the four refusals, each by an input that trips it alone
        tiny = real(1e-40) if prec == 32 else real(1e-60)  # a positive cell whose float scale overflows; ir < 0 keeps r + margin below the limit
        refusals = {
            "grid": ((2, 32, 32), origin, [real(h)] * 3, h),
            "cell": ((64, 32, 32), origin, [real(h), real(-h), real(h)], h),
            "scale": ((64, 32, 32), origin, [real(h), real(h), tiny], real(-1.0)),
            "reach": ((64, 32, 32), origin, [real(0.5 * h), real(h), real(h)], h),
        }
        ans = run(exe, [quant_line(prec, *c) for c in refusals.values()])
        for (name, c), a in zip(refusals.items(), ans):
            s, o, qT, ok = quant_answer(a)
            ws, wo, wqT, wok = quant_formula(real, *c)
            assert (qT, ok) == (0, 0) and not wok, (prec, name, a)
            assert [hx(v) for v in s] == [hx(v) for v in ws], (prec, name, a)
            # alone: which conditions this input fails
            with np.errstate(all="ignore"):
                cs = np.asarray(c[2], real)
                r = (np.float32(real(c[3])) * ws).astype(np.float32)
                failed = {"grid": c[0][0] < 4, "cell": bool((cs <= 0).any()), "scale": bool((~np.isfinite(ws)).any()),
                          "reach": bool((~((r + QP_MARGIN).astype(np.float32) < QP_HALF)).any())}
            assert failed == {k: k == name for k in failed}, (prec, name, failed)
        # three columns are refused like two
        assert quant_answer(run(exe, [quant_line(prec, (3, 32, 32), origin, [real(h)] * 3, h)])[0])[2:] == (0, 0)
    # the reach at its limit (cells of 1: s = 256 and r = 256 ir, both exact): r + margin = 510.5 is accepted, 511 and 511.5 are not
    edge = [quant_line(32, (64, 32, 32), (0, 0, 0), [np.float32(1.0)] * 3, np.float32(v / 256.0)) for v in (508.0, 508.5, 509.0)]
    got = [quant_answer(a)[2:] for a in run(exe, edge)]
    assert got == [(int(np.ceil(510.5 ** 2)) + 1, 1), (0, 0), (0, 0)], got


def test_quantisation_setup_exact(plain, scenes):
    check_quant_setup(plain)
    # the model's threshold() on the model's scenes is the code's qT
    sup, fp = scenes
    todo = [(h, cs, origin) for _, _, h, cs, origin, centre, _ in sup if centre == model.CENTRES[0]] + [fp[2:]]
    ans = run(plain, [quant_line(32, (64, 32, 32), origin, cs, h) for h, cs, origin in todo])
    for (h, cs, origin), a in zip(todo, ans):
        _, _, s = model.quantise(np.zeros((1, 3), np.float32), origin, cs)
        assert quant_answer(a)[2:] == (model.threshold(h, s), 1), (cs, a)
        assert quant_answer(a)[0] == [float(v) for v in s]


# ---- the superset guarantee ----------------------------------------------------------------------------------------------------------
def scene_line(word, prec, f, n, h, cs, origin):
    assert cs[0] == cs[1] == cs[2]
    return "%s %d %s %d %s %s %s" % (word, prec, f, n, hx(h), hx(cs[0]), " ".join(hx(v) for v in origin))


def check_superset(exe, scenes):
    sup, fp = scenes
    for prec in (32, 64):
        ans = run(exe, [scene_line("superset", prec, f, n, h, cs, origin) for f, n, h, cs, origin, _, _ in sup])
        for (f, n, h, cs, origin, centre, cs_over_h), a in zip(sup, ans):
            assert a[0] == "superset" and len(a) == 6, a
            hits, missed, far, qT, ok = (int(t) for t in a[1:])
            print("R%d centre %g cells, cell %g h: %d exact pairs, %d missed, %d owners out of range, qT %d" % (prec, centre, cs_over_h, hits, missed, far, qT))
            _, _, s = model.quantise(np.zeros((1, 3), np.float32), origin, cs)
            assert ok == 1 and qT == model.threshold(h, s)
            assert far == 0, "the scene must stay inside the range the device accepts for owners"
            assert hits > n and missed == 0, (prec, centre, cs_over_h, hits, missed)


def check_false_positives(exe, scenes):
    f, n, h, cs, origin = scenes[1]
    for prec in (32, 64):
        a = run(exe, [scene_line("fprate", prec, f, n, h, cs, origin)])[0]
        assert a[0] == "fprate" and len(a) == 3, a
        exact, kept = int(a[1]), int(a[2])
        print("R%d: %d exact pairs, %d kept by the integer test (%.4f)" % (prec, exact, kept, kept / exact))
        assert exact <= kept <= 1.06 * exact, (prec, exact, kept)


def test_every_exact_hit_passes_the_integer_test(plain, scenes):
    check_superset(plain, scenes)


def test_false_positive_rate_is_a_few_percent(plain, scenes):
    check_false_positives(plain, scenes)


# ---- the window and the small rules -----------------------------------------------------------------------------------------------------
def check_window(exe):
    g = (64, 32, 32)
    cells = 64 * 32 * 32
    for prec in (32, 64):
        cases = [(0, 0), (0, 24), (64, 8), (128, 0), (16, 24), (32, 0), (63, 1)]
        ans = run(exe, ["win %d %d %d %d %d %d" % ((prec,) + g + c) for c in cases])
        got = [[int(t) for t in a[1:]] for a in ans]
        whole = [0, 64, 32, 32, cells, 1]
        assert got[:4] == [whole] * 4, got[:4]          # no window, and windows as wide as the grid or wider: the whole grid, column 0
        assert got[4] == [24, 16, 32, 32, 16 * 32 * 32, 1] and got[5] == [0, 32, 32, 32, 32 * 32 * 32, 1] and got[6] == [1, 63, 32, 32, 63 * 32 * 32, 1], got[4:]


def check_rules(exe):
    values = [0, 1, 2, 3, 4, 6, 64, 96, 2 ** 31, 2 ** 32 - 1]
    ans = run(exe, ["pow2 %d" % v for v in values])
    assert [int(a[1]) for a in ans] == [0, 1, 1, 0, 1, 0, 1, 0, 1, 0]
    grids = [(64, 32, 32), (48, 32, 32), (64, 48, 32), (64, 32, 96), (1, 1, 1), (0, 4, 4)]
    ans = run(exe, ["pow2grid %d %d %d" % g for g in grids])
    assert [int(a[1]) for a in ans] == [1, 0, 0, 0, 1, 0]
    blocks = [0, 1, 15, 16, 31, 32, 160, 16383, 16384, 16400, 10 ** 6]   # one wall workgroup per 16 interior ones, from 1 to 1024
    ans = run(exe, ["wallblocks %d" % b for b in blocks])
    assert [int(a[1]) for a in ans] == [1, 1, 1, 1, 1, 2, 10, 1023, 1024, 1024, 1024]


def test_window(plain):
    check_window(plain)


def test_small_rules(plain):
    check_rules(plain)


def test_under_sanitizers(sanitized, scenes):
    check_thresholds(sanitized)
    check_quant_setup(sanitized)
    check_window(sanitized)
    check_rules(sanitized)
    check_superset(sanitized, scenes)
    check_false_positives(sanitized, scenes)
