"""What differs by solver on the host (nereus_amd/csrc/nrs_host_solver.h) without a GPU, through the program of
tests/test_host_parts_cpu.py (tests/host_parts_main.cpp), plain and under -fsanitize=address,undefined.

Every expectation restates the rule of the commit before the header existed, from its nrs_ctx_impl.h (Ctx::step, set_params,
pcisph_prepare, pbf_prepare, dfsph_prepare, prototype_sums, init, array, get_stat); nothing is read from the code under test.

  * stage: every solver x every stage 0 .. NRS_STAGE_COUNT.
  * stale: each of the seven key fields changed alone, in pairs and to NaN (on one side, and on both: NaN != NaN).
  * delta, eps, thr, spacing: hex-float exact in both precisions, on ordinary inputs and on the failing ones (zero neighbours,
    non-finite delta, eps <= 0, D <= 0, spacing 0 / negative / NaN / h / sp > 64, h <= 0) with their texts.
  * buffers: per solver the allocation list, its units and which are zero-filled, in order.
  * array: 5 solvers x ids -1 .. 40 x midStep x walls x bodies x the 16 validity combinations x pciXs (53,760 cases): code, full text,
    buffer and unit.
  * stat: 5 solvers x ids -1 .. 13 x packed x pending x solved x dfDenN, dfDivN in {0, 7} x the 8 hit-list facts (19,200 cases): code,
    full text, what to compute, which error buffer and count.
"""
import itertools

import numpy as np
import pytest

from tests.test_host_parts_cpu import cmd, plain, refusal, run, sanitized  # noqa: F401  (plain, sanitized: fixtures)

E_INVALID, E_STATE = -1, -4
SESPH, IISPH, PCISPH, PBF, DFSPH = range(5)
SOLVERS = (SESPH, IISPH, PCISPH, PBF, DFSPH)
PREDICTIVE = {PCISPH: "PCISPH", PBF: "PBF", DFSPH: "DFSPH"}
STAGE_DENSITY, STAGE_P_ADVECT, STAGE_P_INTEGRATE, STAGE_COUNT = 4, 7, 9, 16


# ---- stage ---------------------------------------------------------------------------------------------------------------------------
def stage_model(solver, stop):
    """Ctx::step of the commit before"""
    name = PREDICTIVE.get(solver)
    if name and stop and not (stop <= STAGE_DENSITY or STAGE_P_ADVECT <= stop <= STAGE_P_INTEGRATE):
        return E_INVALID, "stage not part of a %s step (HASH .. DENSITY, P_ADVECT .. P_INTEGRATE)" % name
    return 0, ""


def check_stage(exe):
    cases = [(s, k) for s in SOLVERS for k in range(STAGE_COUNT + 1)]
    ans = run(exe, [cmd("stage", s, k) for s, k in cases])
    refused = 0
    for (s, k), a in zip(cases, ans):
        assert refusal(a) == stage_model(s, k), (s, k)
        refused += refusal(a)[0] != 0
    assert refused == 3 * (2 + STAGE_COUNT - STAGE_P_INTEGRATE)  # FORCES, INTEGRATE and the I_ stages up to the count, per predictive solver


def test_stage(plain):
    check_stage(plain)


# ---- stale ---------------------------------------------------------------------------------------------------------------------------
KEY = ("timestep", "particleMass", "restDensity", "interactionRadius", "kpoly", "kpoly_grad", "kpress_grad")
KEY0 = (1e-3, 0.02, 1000.0, 0.0457, 2.5e6, -7.5e7, -1.2e8)


def stale_model(o, q):
    """Ctx::set_params of the commit before: != on each field (NaN differs from everything, itself included)"""
    d = {k: a != b for k, a, b in zip(KEY, o, q)}
    delta = d["timestep"] or d["particleMass"] or d["restDensity"] or d["interactionRadius"] or d["kpoly_grad"]
    eps = d["particleMass"] or d["restDensity"] or d["interactionRadius"] or d["kpress_grad"]
    wq = d["interactionRadius"] or d["kpoly"]
    return "%d %d %d %d" % (delta, eps, eps, wq)


def stale_cases():
    nan = float("nan")
    cases = [(KEY0, KEY0)]
    for i in range(7):
        q = list(KEY0)
        q[i] = KEY0[i] * 1.5
        cases.append((KEY0, tuple(q)))
        for v in (nan, float("inf"), -KEY0[i], 0.0):
            q = list(KEY0)
            q[i] = v
            cases += [(KEY0, tuple(q)), (tuple(q), KEY0), (tuple(q), tuple(q))]
    for i, j in itertools.combinations(range(7), 2):
        q = list(KEY0)
        q[i], q[j] = KEY0[i] * 0.5, KEY0[j] * 2.0
        cases.append((KEY0, tuple(q)))
        q[j] = nan
        cases.append((KEY0, tuple(q)))
    return cases


def check_stale(exe):
    cases = stale_cases()
    ans = run(exe, [cmd("stale", o, q) for o, q in cases])
    seen = set()
    for (o, q), a in zip(cases, ans):
        assert a == ("stale", stale_model(o, q)), (o, q, a)
        seen.add(a[1])
    # nothing, each constant's own field alone (dt / kpoly_grad, kpress_grad, kpoly), the shared ones, and the pairs
    assert seen >= {"0 0 0 0", "1 0 0 0", "0 1 1 0", "0 0 0 1", "1 1 1 0", "1 1 1 1", "1 0 0 1", "0 1 1 1"}


def test_stale(plain):
    check_stale(plain)


# ---- the derived constants -----------------------------------------------------------------------------------------------------------
H, SP = 0.0457, 0.027144176165949066
O_PCI = (1.25e-3, -3.5e-4, 7.75e-4, 1.9e9, 56.0)   # (|sum g| small against sum g . g, as on a lattice)
O_PBF = (3.0e-6, -2.0e-6, 1.0e-6, 2.3e-3, 56.0)
O_SETS = [O_PCI, O_PBF, (0.0, 0.0, 0.0, 1.0, 1.0), (1e200, 0.0, 0.0, 1.0, 3.0), (0.0, 0.0, 0.0, 0.0, 5.0), (float("nan"), 0.0, 0.0, 1.0, 2.0),
          (0.0, 0.0, 0.0, -1.0, 2.0), (1.0, 2.0, 3.0, 4.0, 0.0), (0.0, 0.0, 0.0, 1e-320, 1.0), (0.0, 0.0, 0.0, 1e300, 1.0)]


def rounded(v, prec):
    with np.errstate(all="ignore"):
        return float(np.float32(v)) if prec == 32 else float(v)


def no_neighbour(o, sp, h, who, what):
    if o[4] == 0.0:
        return E_INVALID, "%s: the prototype particle (lattice spacing %g, h %g) has no neighbour within h: no %s" % (who, sp, h, what)
    return None


def proto_d(o):
    return o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3]


def delta_model(prec, given, o, sp, h, dt, m, rho0):
    """Ctx::pcisph_prepare + prototype_sums of the commit before"""
    if given > 0.0:
        return 0, rounded(given, prec)
    r = no_neighbour(o, sp, h, "PCISPH", "pressure scale delta")
    if r:
        return r
    with np.errstate(all="ignore"):
        q = np.float64(dt) * np.float64(m) / np.float64(rho0)
        beta = 2.0 * q * q
        d = float(np.float64(-1.0) / (beta * (-(np.float64(o[0]) * o[0] + np.float64(o[1]) * o[1] + np.float64(o[2]) * o[2]) - o[3])))
    if not np.isfinite(d):
        return E_INVALID, "PCISPH: the prototype gives no finite pressure scale delta"
    return 0, rounded(d, prec)


def eps_model(prec, relax, o, sp, h):
    """Ctx::pbf_prepare + pbf_prototype_d of the commit before"""
    r = no_neighbour(o, sp, h, "PBF", "eps")
    if r:
        return r
    with np.errstate(all="ignore"):
        e = float(np.float64(relax) * np.float64(proto_d(np.array(o, np.float64))))
    if not (e > 0.0) or not np.isfinite(e):
        return E_INVALID, "PBF: the prototype gives no finite positive eps"
    return 0, rounded(e, prec)


def thr_model(prec, o, sp, h):
    """Ctx::dfsph_prepare of the commit before"""
    r = no_neighbour(o, sp, h, "DFSPH", "D_proto")
    if r:
        return r
    with np.errstate(all="ignore"):
        d = float(proto_d(np.array(o, np.float64)))
    if not (d > 0.0) or not np.isfinite(d):
        return E_INVALID, "DFSPH: the prototype gives no finite positive D_proto"
    with np.errstate(all="ignore"):
        return 0, rounded(1e-6 * d, prec)


def spacing_model(prec, sp, h, who):
    """Ctx::prototype_sums of the commit before: the spacing is rounded to SReal first"""
    sp = rounded(sp, prec)
    with np.errstate(all="ignore"):
        if not (sp > 0.0) or not np.isfinite(sp) or not (h > 0.0) or float(np.float64(h) / np.float64(sp)) > 64.0:
            return E_INVALID, "%s: the prototype spacing (default cbrt(m / rho0)) must be positive and at least h / 64" % who
        return 0, int(np.ceil(np.float64(h) / np.float64(sp))) + 1


def value_answer(a):
    """(code, value or text) of an answer "rc 0 VALUE" / "rc CODE TEXT" """
    code, msg = refusal(a)
    if code:
        return code, msg
    return 0, (float.fromhex(msg) if "x" in msg else (int(msg) if msg.lstrip("-").isdigit() else float(msg)))


def same(got, want):
    if got[0] != want[0]:
        return False
    if got[0] or isinstance(want[1], int):
        return got[1] == want[1]
    return got[1] == want[1] or (got[1] != got[1] and want[1] != want[1])  # (hex-float exact; NaN as NaN)


def derived_cases():
    cases = []
    for prec in (32, 64):
        for o in O_SETS:
            for given in (0.0, 812.25, 1e-50):   # (1e-50 rounds to 0 in fp32: a given delta is taken as it is)
                for dt, m, rho0 in ((1e-3, 0.02, 1000.0), (0.0, 0.02, 1000.0), (1e-3, 0.02, 0.0), (1e-160, 1e-160, 1.0)):
                    cases.append((cmd("delta", prec, given, o, SP, H, dt, m, rho0), delta_model(prec, given, o, SP, H, dt, m, rho0)))
            for relax in (0.01, 1.0, 0.0, -1.0, 1e308, float("nan")):
                cases.append((cmd("eps", prec, relax, o, SP, H), eps_model(prec, relax, o, SP, H)))
            cases.append((cmd("thr", prec, o, SP, H), thr_model(prec, o, SP, H)))
        for who, name in enumerate(("PCISPH", "PBF", "DFSPH")):
            for sp, h in ((SP, H), (H, H), (H / 64.0, H), (H / 64.000001, H), (H / 63.5, H), (0.0, H), (-SP, H), (float("nan"), H), (float("inf"), H),
                          (1e-46, H), (SP, 0.0), (SP, -H), (SP, float("nan")), (2.0 * H, H), (H / 3.0, H), (0.1, 0.3), (0.1, 0.30000001)):
                cases.append((cmd("spacing", prec, sp, h, who), spacing_model(prec, sp, h, name)))
    return cases


def check_derived(exe):
    cases = derived_cases()
    ans = run(exe, [c for c, _ in cases])
    assert len(ans) == len(cases)
    texts = set()
    for (c, want), a in zip(cases, ans):
        got = value_answer(a)
        assert same(got, want), (c, got, want)
        if got[0]:
            texts.add(got[1].split(":")[0] + ":" + got[1].split(":")[1][:24])
    # every failing branch was reached: no neighbour (x3), non-finite delta, eps, D_proto, the spacing (x3)
    assert len(texts) == 9, texts


def test_derived_constants(plain):
    check_derived(plain)


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
# Ctx::init of the commit before: per solver the allocations in order, (name, unit); then the names that are zero-filled, in order
INIT = {
    SESPH: ([], []),
    IISPH: ([("inv", "u"), ("densAdv", "s"), ("densCorr", "s"), ("P_l", "s"), ("P_l2", "s"), ("aii", "s"), ("velAdv", "v"), ("forcesAdv", "v"),
             ("forcesP", "v"), ("diiF", "v"), ("diiB", "v"), ("sumDij", "v"), ("diiSum", "v")],
            ["densAdv", "densCorr", "P_l", "P_l2", "aii", "velAdv", "forcesAdv", "forcesP", "diiF", "diiB", "sumDij"]),
    PCISPH: ([("velAdv", "v"), ("forcesAdv", "v"), ("forcesP", "v"), ("densCorr", "s"), ("P_l", "s"), ("posPred", "v"), ("posPred2", "v"),
              ("pciErr", "s")], ["velAdv", "forcesAdv", "forcesP", "densCorr", "P_l", "posPred", "posPred2", "pciErr"]),
    DFSPH: ([("velAdv", "v"), ("forcesAdv", "v"), ("forcesP", "v"), ("densCorr", "s"), ("P_l", "s"), ("posPred", "v"), ("pciErr", "s"),
             ("dfAlpha", "s"), ("dfKvA", "s"), ("dfKvB", "s"), ("dfErrV", "s")],
            ["velAdv", "forcesAdv", "forcesP", "densCorr", "P_l", "posPred", "pciErr", "dfAlpha", "dfKvA", "dfKvB", "dfErrV"]),
}
INIT[PBF] = INIT[PCISPH]


def check_buffers(exe):
    ans = run(exe, [cmd("buffers", s) for s in SOLVERS])
    for s, a in zip(SOLVERS, ans):
        assert a[0] == "buffers"
        got = [t.split(":") for t in a[1].split()]
        alloc, zeroed = INIT[s]
        assert [(n, u) for n, u, _ in got] == alloc, s
        assert [n for n, _, z in got if z == "1"] == zeroed, s


def test_buffers(plain):
    check_buffers(plain)


# ---- array ---------------------------------------------------------------------------------------------------------------------------
(A_POS, A_VEL, A_PRESSURE, A_HASH, A_INDEX, A_CELL_START, A_CELL_END, A_SORTED_POS, A_SORTED_VEL, A_DENS, A_PRES, A_FORCES, A_B_HASH, A_B_INDEX,
 A_B_CELL_START, A_B_CELL_END, A_B_SORTED) = range(17)
(A_DENS_ADV, A_DENS_CORR, A_P_L, A_AII, A_VEL_ADV, A_FORCES_ADV, A_FORCES_P, A_DII_FLUID, A_DII_BOUNDARY, A_SUM_DIJ, A_POS_PRED, A_VORTICITY,
 A_DFSPH_ALPHA, A_DFSPH_KAPPA_V, A_NORMALS, A_B_BODY) = range(20, 36)
PLAIN_ARRAYS = {A_POS: ("posA", "v"), A_VEL: ("velA", "v"), A_PRESSURE: ("presA", "s"), A_HASH: ("hashCur", "u"), A_INDEX: ("indexCur", "u"),
                A_CELL_START: ("cellStart", "c"), A_CELL_END: ("cellEnd", "c"), A_DENS: ("dens", "s"), A_FORCES: ("forces", "v"),
                A_B_HASH: ("bHashCur", "ub"), A_B_INDEX: ("bIndexCur", "ub"), A_B_SORTED: ("bSorted", "vb"), A_DENS_ADV: ("densAdv", "s"),
                A_DENS_CORR: ("densCorr", "s"), A_P_L: ("P_l", "s"), A_AII: ("aii", "s"), A_VEL_ADV: ("velAdv", "v"),
                A_FORCES_ADV: ("forcesAdv", "v"), A_FORCES_P: ("forcesP", "v"), A_DII_FLUID: ("diiF", "v"), A_DII_BOUNDARY: ("diiB", "v"),
                A_SUM_DIJ: ("sumDij", "v")}


def array_model(solver, which, mid, walls, bodies, vort, normals, alpha, kv, xs):
    """Ctx::array of the commit before: the switch, then the refusals behind it, in its order.  (code, text, buffer, unit)"""
    sesph, pcisph, pbf, dfsph = solver == SESPH, solver == PCISPH, solver == PBF, solver == DFSPH
    cur = not mid

    def no(code, text):
        return code, text, "-", "-"

    if which in PLAIN_ARRAYS:
        p = PLAIN_ARRAYS[which]
    elif which == A_SORTED_POS:
        p = ("posA" if cur else "posB", "v")
    elif which == A_SORTED_VEL:
        p = ("velA" if cur else "velB", "v")
    elif which == A_PRES:
        p = ("presA" if (solver in (IISPH, PCISPH, PBF, DFSPH) and cur) else "presB", "s")
    elif which == A_B_CELL_START:
        p = ("bCellStart", "c") if walls else ("none", "0")
    elif which == A_B_CELL_END:
        p = ("bCellEnd", "c") if walls else ("none", "0")
    elif which == A_POS_PRED:
        p = ("posPred2" if xs else "posPred", "v")
    elif which == A_VORTICITY:
        if not pbf:
            return no(E_STATE, "PBF array requested from another context")
        if not vort:
            return no(E_STATE, "no PBF step with vorticity confinement yet")
        p = ("pbfVort", "v")
    elif which == A_NORMALS:
        if not (pcisph or pbf or dfsph):
            return no(E_STATE, "Akinci array requested from a SESPH or IISPH context")
        if not normals:
            return no(E_STATE, "no step with Akinci surface tension (gamma > 0) yet")
        p = ("akNormals", "v")
    elif which == A_B_BODY:
        if not bodies:
            return no(E_STATE, "no boundary body assignment (nrs_set_boundary_bodies)")
        return 0, "", "bdBodySorted", "ub"
    elif which in (A_DFSPH_ALPHA, A_DFSPH_KAPPA_V):
        if not dfsph:
            return no(E_STATE, "DFSPH array requested from another context")
        if which == A_DFSPH_ALPHA:
            if not alpha:
                return no(E_STATE, "no DFSPH factor launch yet")
            p = ("dfAlpha", "s")
        else:
            if not kv:
                return no(E_STATE, "no DFSPH step yet")
            p = ("dfKvA" if cur else "dfKvB", "s")
    else:
        return no(E_INVALID, "unknown array id")
    if which == A_POS_PRED and not pcisph and not pbf:
        return no(E_STATE, "PCISPH / PBF array requested from another context")
    pci_array = which in (A_VEL_ADV, A_FORCES_ADV, A_FORCES_P, A_DENS_CORR, A_P_L, A_POS_PRED, A_VORTICITY, A_NORMALS)
    if pcisph and which >= A_DENS_ADV and not pci_array:
        return no(E_STATE, "IISPH array requested from a PCISPH context")
    if pbf and which >= A_DENS_ADV and not pci_array:
        return no(E_STATE, "IISPH array requested from a PBF context")
    df_array = which in (A_VEL_ADV, A_FORCES_ADV, A_FORCES_P, A_DENS_CORR, A_P_L, A_DFSPH_ALPHA, A_DFSPH_KAPPA_V, A_NORMALS)
    if dfsph and which >= A_DENS_ADV and not df_array:
        return no(E_STATE, "IISPH / PCISPH / PBF array requested from a DFSPH context")
    if which >= A_DENS_ADV and sesph:
        return no(E_STATE, "IISPH array requested from a SESPH context")
    return 0, "", p[0], p[1]


def parse_route(line):
    """a line "code a b ... | text" of the array / stat commands -> (code, text, a, b, ...)"""
    head, _, text = " ".join(line).partition(" |")
    f = head.split()
    return (int(f[0]), text.strip()) + tuple(f[1:])


def check_array(exe):
    ans = run(exe, [cmd("array", s) for s in SOLVERS])
    per = 42 * 2 * 2 * 2 * 16 * 2
    assert len(ans) == 5 * (per + 1)
    texts = set()
    for k, s in enumerate(SOLVERS):
        block = ans[k * (per + 1):(k + 1) * (per + 1)]
        assert block[-1] == ("array", "done")
        it = iter(block)
        for which in range(-1, 41):
            for mid, walls, bodies in itertools.product((0, 1), repeat=3):
                for m in range(16):
                    for xs in (0, 1):
                        got = parse_route(next(it))
                        want = array_model(s, which, mid, walls, bodies, m & 1, m & 2, m & 4, m & 8, xs)
                        assert got == want, (s, which, mid, walls, bodies, m, xs, got, want)
                        texts.add(want[1])
    assert len(texts) == 15  # "", and every one of the fourteen refusals


def test_array_routing(plain):
    check_array(plain)


def test_array_examples():
    """the two the issue names, on the model itself"""
    assert array_model(SESPH, A_VORTICITY, 0, 1, 0, 1, 1, 1, 1, 0)[1] == "PBF array requested from another context"
    for s in (DFSPH, IISPH):
        assert array_model(s, A_POS_PRED, 0, 1, 0, 1, 1, 1, 1, 0)[1] == "PCISPH / PBF array requested from another context"
    assert array_model(SESPH, A_B_BODY, 0, 1, 1, 0, 0, 0, 0, 0) == (0, "", "bdBodySorted", "ub")


# ---- stat ----------------------------------------------------------------------------------------------------------------------------
(S_MOVERS, S_HIT_OVERFLOW, S_HIT_MEAN, S_HIT_MAX, S_UNSTAGED, S_DENSITY_ERROR, S_PCISPH_DELTA, S_PBF_EPSILON, S_DFSPH_DENSITY_AVG,
 S_DFSPH_DIVERGENCE_AVG, S_DFSPH_DIVERGENCE_ITERATIONS, S_SLAB_PARTITION) = range(12)


def stat_model(solver, which, packed, pending, solved, den, div, hit_counts, particles, mid):
    """Ctx::get_stat of the commit before, up to the device work: (code, text, what, divergence buffer?, count, form the max first?).
    On a PBF context with a pending fixed-count maximum the commit before formed it first and tested "no PBF solve yet" on the
    result: the last field says form it, then ask again (with pending = 0 and solved as the maximum leaves it)."""
    pcisph, pbf, dfsph = solver == PCISPH, solver == PBF, solver == DFSPH

    def no(code, text):
        return code, text, "-", "0", "0", "0"

    def ok(what, dv=0, count=0, form=0):
        return 0, "", what, str(dv), str(count), str(form)

    if which == S_MOVERS:
        return ok("movers")
    if which == S_SLAB_PARTITION:
        return ok("slabForm") if packed else no(E_STATE, "no nrs_slab_pack yet")
    if pbf and which in (S_DENSITY_ERROR, S_PBF_EPSILON):
        if not pending and not solved:
            return no(E_STATE, "no PBF solve yet")
        return ok("pbfError" if which == S_DENSITY_ERROR else "pbfEps", form=int(bool(pending)))
    if which in (S_DFSPH_DENSITY_AVG, S_DFSPH_DIVERGENCE_AVG, S_DFSPH_DIVERGENCE_ITERATIONS) or (dfsph and which == S_DENSITY_ERROR):
        if not dfsph:
            return no(E_STATE, "DFSPH statistic requested from another context")
        if which == S_DFSPH_DIVERGENCE_ITERATIONS:
            return ok("dfDivIters")
        dv = which == S_DFSPH_DIVERGENCE_AVG
        cnt = div if dv else den
        if not cnt:
            return no(E_STATE, "no DFSPH divergence solve yet (or it is off)" if dv else "no DFSPH density solve yet")
        return ok("dfMax" if which == S_DENSITY_ERROR else "dfAvg", int(dv), cnt)
    if which in (S_DENSITY_ERROR, S_PCISPH_DELTA):
        if not pcisph:
            return no(E_STATE, "PCISPH statistic requested from another context")
        if not solved:
            return no(E_STATE, "no PCISPH solve yet")
        return ok("pciError" if which == S_DENSITY_ERROR else "pciDelta")
    if which == S_PBF_EPSILON:
        return no(E_STATE, "PBF statistic requested from another context")
    if which not in (S_HIT_OVERFLOW, S_HIT_MEAN, S_HIT_MAX, S_UNSTAGED):
        return no(E_INVALID, "unknown statistic")
    if not hit_counts or not particles or mid:
        return no(E_STATE, "no shared hit lists (reference-order kernels, or no step yet)")
    return ok({S_HIT_OVERFLOW: "hitOverflow", S_HIT_MEAN: "hitMean", S_HIT_MAX: "hitMax", S_UNSTAGED: "unstaged"}[which])


def check_stat(exe):
    ans = run(exe, [cmd("stat", s) for s in SOLVERS])
    per = 15 * 2 * 2 * 2 * 2 * 2 * 8
    assert len(ans) == 5 * (per + 1)
    texts, kinds = set(), set()
    for k, s in enumerate(SOLVERS):
        block = ans[k * (per + 1):(k + 1) * (per + 1)]
        assert block[-1] == ("stat", "done")
        it = iter(block)
        for which in range(-1, 14):
            for packed, pending, solved in itertools.product((0, 1), repeat=3):
                for den in (0, 7):
                    for div in (0, 7):
                        for m in range(8):
                            got = parse_route(next(it))
                            want = stat_model(s, which, packed, pending, solved, den, div, m & 1, m & 2, m & 4)
                            assert got == want, (s, which, packed, pending, solved, den, div, m, got, want)
                            texts.add(want[1])
                            kinds.add(want[2])
    assert len(texts) == 11 and len(kinds) == 14  # "" and the ten refusals; "-" and the thirteen things to compute


def test_stat_routing(plain):
    check_stat(plain)


# ---- IISPH's exit rule ---------------------------------------------------------------------------------------------------------------
def iisph_loop_model(prec, n, max_iters, watch, flag_from, accs):
    """The loop of Ctx::iisph_tail_once of the commit before (pressureSolve, sph_cuda.cu:702-899), in the context's precision:
    (iterations, word seen set, the measure calls).  A call is "r" (the sum) and / or "f" (the watch word, 1 from iteration flag_from
    on) followed by the iterations done when it was made."""
    real = np.float32 if prec == 32 else np.float64
    l, k, hflag, flag_read, calls = 0, 0, 0, False, []
    rho_avg, rd, max_rho_err = real(0.0), real(1000.0), real(1.0)
    while (real(rho_avg - rd) > max_rho_err) or l < 2:
        l += 1                                   # one iteration
        flag_read = False
        if max_iters and l >= max_iters:
            break
        if l >= 2:                               # (the average of the first iteration is never looked at: nothing is reduced)
            if watch:                            # (the word rides in the reduction's round trip)
                hflag = int(bool(flag_from) and l >= flag_from)
            calls.append(("rf" if watch else "r") + str(l))
            acc = accs[min(k, len(accs) - 1)]
            k += 1
            flag_read = True
            if watch and hflag:
                break
            rho_avg = real(acc)                  # (R)acc, then / N in R
            rho_avg = real(rho_avg / real(n))
    if watch and not flag_read:                  # the last iteration did no reduction: the word alone
        hflag = int(bool(flag_from) and l >= flag_from)
        calls.append("f" + str(l))
    return l, int(bool(watch and hflag)), calls


def iisph_loop_cases():
    n = 1000
    slow = [n * v for v in (1010.0, 1005.0, 1001.5, 1000.9)]          # the error bound is met by the fourth reduction: l = 5
    never = [n * 1500.0]
    cases = []
    for prec in (32, 64):
        for watch in (0, 1):
            cases.append((prec, n, 0, watch, 0, [n * 1000.5]))        # exit at l = 2
            cases.append((prec, n, 0, watch, 0, [n * 1001.0]))        # (rho_avg - 1000 == 1 is not > 1)
            cases.append((prec, n, 0, watch, 0, slow))                # exit on the error bound
            cases.append((prec, n, 9, watch, 0, slow))                # ... before the cap
            for cap in (1, 2, 3, 5, 7):                               # exit at maxIters = 1, 2, n: no reduction behind the last iteration
                cases.append((prec, n, cap, watch, 0, never))
            for flag_from in (1, 2, 3, 4):                            # the word set in a reduction round
                cases.append((prec, n, 0 if watch else 8, watch, flag_from, never))   # (unwatched, only the cap ends it)
                cases.append((prec, n, 6, watch, flag_from, slow))
            for cap, flag_from in ((1, 1), (2, 1), (2, 2), (4, 4), (3, 4)):   # ... and where no reduction ran (or not yet: (3, 4))
                cases.append((prec, n, cap, watch, flag_from, never))
        # rounding of the average: (R)acc / N in R.  Sums whose average straddles 1001 in double and rounds onto it in float
        for big_n in (3, 1000, 16777217, 100000007):
            for eps in (-3e-7, -1e-9, 0.0, 1e-9, 3e-7, 1e-4):
                cases.append((prec, big_n, 0, 0, 0, [big_n * 1001.0 * (1.0 + eps), big_n * 1000.0]))
    return cases


def check_iisph_loop(exe):
    cases = iisph_loop_cases()
    ans = run(exe, [cmd("iloop", prec, n, cap, watch, flag_from, accs) for prec, n, cap, watch, flag_from, accs in cases])
    assert len(ans) == 2 * len(cases)
    by_prec, seen = {}, set()
    for k, c in enumerate(cases):
        prec, n, cap, watch, flag_from, accs = c
        iters, flagged, calls = iisph_loop_model(prec, n, cap, watch, flag_from, accs)
        v = ans[2 * k + 1][1].split()
        assert refusal(ans[2 * k]) == (0, "") and ans[2 * k + 1][0] == "iloop", (c, ans[2 * k])
        assert (int(v[0]), int(v[1]), int(v[2]), v[3:]) == (iters, iters, flagged, calls), (c, v, iters, flagged, calls)
        assert not any(t.lstrip("rf") == "1" and "r" in t for t in calls)           # no reduction before l >= 2
        assert sum(t.startswith("f") for t in calls) <= 1 and (not watch) == (not any("f" in t for t in calls))
        by_prec.setdefault((n, cap, watch, flag_from, tuple(accs)), {})[prec] = iters
        seen.add((iters == 2, bool(cap) and iters == cap, flagged, bool(calls) and calls[-1].startswith("f")))
    assert any(len(set(d.values())) == 2 for d in by_prec.values())                  # float and double round the average apart
    assert {s[0] for s in seen} == {s[1] for s in seen} == {s[3] for s in seen} == {False, True} and {s[2] for s in seen} == {0, 1}
    assert any(s[2] and s[3] for s in seen) and any(s[2] and not s[3] for s in seen)  # the word found late, and in a reduction round


def test_iisph_loop(plain):
    check_iisph_loop(plain)


def test_iisph_loop_model_examples():
    """the rule on the model itself: the cases the exit rule is known by"""
    n = 1000
    assert iisph_loop_model(32, n, 0, 0, 0, [n * 1000.5]) == (2, 0, ["r2"])
    assert iisph_loop_model(64, n, 0, 1, 0, [n * 1010.0, n * 1005.0, n * 1001.5, n * 1000.9]) == (5, 0, ["rf2", "rf3", "rf4", "rf5"])
    assert iisph_loop_model(32, n, 1, 1, 1, [0.0]) == (1, 1, ["f1"])
    assert iisph_loop_model(32, n, 2, 1, 0, [0.0]) == (2, 0, ["f2"])
    assert iisph_loop_model(64, n, 5, 1, 0, [n * 1500.0]) == (5, 0, ["rf2", "rf3", "rf4", "f5"])
    assert iisph_loop_model(64, n, 0, 1, 3, [n * 1500.0]) == (3, 1, ["rf2", "rf3"])
    assert iisph_loop_model(64, n, 0, 0, 3, [n * 1500.0, n * 1500.0, n * 1000.0]) == (4, 0, ["r2", "r3", "r4"])


# ---- everything once more under the sanitizers ---------------------------------------------------------------------------------------
def test_sanitized(sanitized):
    check_iisph_loop(sanitized)
    check_stage(sanitized)
    check_stale(sanitized)
    check_derived(sanitized)
    check_buffers(sanitized)
    check_array(sanitized)
    check_stat(sanitized)
