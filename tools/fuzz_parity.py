"""Randomised parity soak (GPU box): production kernels against the reference-order kernels, bit for bit, on random particle clouds
with random grid geometry (cell size != h, anisotropic, origins far from the particles), optional random wall sheets; every 7th
seed in fp64, every 3rd with the Monaghan kernels, every 5th IISPH; every 13th on a grid one or two cells wide in x (no quantised
scan), every 17th with the grid origin more than 4096 cells away (beyond the quanta's error budget), every 19th with NaN / inf
coordinates.
With a solver named (pcisph / pbf / dfsph), the same scenes run that solver instead (PBF with random loop, XSPH, tensile and vorticity
settings, DFSPH with random settings of both loops and the warm start), production against reference order at the advection stage, at
the solve stage and after 3 (6) steps; pcisph-model / pbf-model / dfsph-model compare the device with the float64 models of tests/ on
pieces of those scenes, of the geometry where both find the same pairs (one_vs_model).
With a flag set named (staged, staged+nofusion, staged+fullsort, fast, fast+staged), the same scenes run as fp32 Muller SESPH with
NRS_FLAG_STAGED_SCAN / NRS_FLAG_FAST_ARITH (one_flags): the exact sets against the reference order bit for bit, the FAST sets against
the CPU oracle within the mode's bar.
With a reader named (sample, surface, aniso, diffuse, track), unscaled pieces of the same scenes (make_reader_scene: cell edges >= h,
grid axes >= 4 cells, the clumps, far origins, wrap and NaN / inf rows kept; no step is taken) are read out by the field sampler, the
surface mesher, the anisotropic passes, the diffuse step and nrs_track_diffuse and compared with the models of tests/ (one_sample,
one_surface, one_aniso, one_diffuse, one_track_diffuse).
usage: python tools/fuzz_parity.py [seeds=100] [first=0] [oracle | pcisph | pbf | dfsph | pcisph-model | pbf-model | dfsph-model | <flag set> | <reader>]
  (oracle: compare with the CPU oracle instead (one_vs_oracle): keys bit-exact, floats within the precision's parity bars, NaN-aware)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nereus_amd import capi
from nereus_amd.params import default_params

SOLVERS = {"pcisph": capi.PCISPH, "pbf": capi.PBF, "dfsph": capi.DFSPH}


def make_scene(seed, solver=None, config=None):
    """solver None: SESPH or IISPH by seed, as the soak has always drawn them.  PCISPH / PBF: the same scene (the same draws, in the same
    order) with the IISPH constructor's parameters on every 5th seed, and the settings of the loop drawn after all of them.
    config: optional dict with any of solver (SESPH / IISPH), double, kset replacing what the seed decides for them; every random draw
    stays the same (None: the scenes the soak has always drawn)."""
    rng = np.random.default_rng(seed)
    drawn = capi.IISPH if seed % 5 == 4 else capi.SESPH
    double, kset = (seed % 7 == 6), (0 if seed % 3 == 2 else 1)
    if config:
        drawn, double, kset = config.get("solver", drawn), bool(config.get("double", double)), int(config.get("kset", kset))
    solver = drawn if solver is None else solver
    p = default_params(1 if drawn == capi.IISPH else 0, double=double).copy()
    real = np.float64 if double else np.float32
    h = float(p["interactionRadius"][0])
    n = int(rng.integers(500, 30000))
    if seed % 11 == 10:  # large enough for the coherent re-sort (merge path) of the production steps
        n = int(rng.integers(40000, 150000))
    ext = rng.uniform(4, 30, 3) * h * np.array([1.0, rng.uniform(0.3, 1.0), rng.uniform(0.3, 1.0)])
    centre = rng.uniform(-0.5, 0.5, 3)
    pos = np.ones((n, 4), real)
    dens_mode = rng.integers(0, 3)
    if dens_mode == 0:
        pos[:, :3] = centre + rng.uniform(-0.5, 0.5, (n, 3)) * ext
    elif dens_mode == 1:   # clumps
        c = centre + rng.uniform(-0.5, 0.5, (8, 3)) * ext
        pos[:, :3] = c[rng.integers(0, 8, n)] + rng.normal(0, 1.2 * h, (n, 3))
    else:                  # jittered lattice
        m = int(round(n ** (1 / 3))) + 1
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        pos[:, :3] = centre + (g - m / 2) * (0.85 * h) + rng.normal(0, 0.03 * h, (n, 3))
    vel = np.zeros_like(pos); vel[:, :3] = rng.normal(0, 0.5, (n, 3))
    # grid geometry
    cs = h * np.array([rng.choice([1.0, 1.0, 1.25, 0.62]), rng.choice([1.0, 1.0, 1.4]), rng.choice([1.0, 1.0, 0.8])])
    p["cellSize"][0] = cs.astype(real)
    lo = pos[:, :3].min(0) - rng.uniform(0.05, 40.0) * h
    far = seed % 17 == 16   # the cloud sits > 4096 cells from the grid origin on one axis: outside the quantised scan's error budget
    if far:                 # (QP_FAR) — owners are diverted to the wall workgroups' exact scan / the reference-order walk
        lo[int(rng.integers(0, 3))] -= rng.uniform(4200, 9000) * cs.max()
    p["worldOrigin"][0] = lo.astype(real)
    gs = [int(2 ** np.ceil(np.log2(max(4, (pos[:, a].max() - lo[a]) / cs[a] + 2)))) for a in range(3)]
    if rng.random() < 0.3: gs[int(rng.integers(0, 3))] //= 2      # particles beyond the grid: wrap
    gs = [min(max(g, 4 if a == 0 else 1), 1024) for a, g in enumerate(gs)]
    if seed % 13 == 12: gs[0] = int(rng.choice([1, 2]))          # x grids narrower than 4 cells: no quantised scan, no hit lists (qOk false)
    while gs[0] * gs[1] * gs[2] > 2 ** 27: gs[int(np.argmax(gs))] //= 2
    p["gridSize"][0] = gs; p["numCells"][0] = gs[0] * gs[1] * gs[2]
    bi = vbi = None
    if rng.random() < 0.6:
        nb = int(rng.integers(200, 6000))
        bi = np.ones((nb, 4), real)
        bi[:, :3] = centre + rng.uniform(-0.5, 0.5, (nb, 3)) * ext
        bi[:, int(rng.integers(0, 3))] = real(pos[:, :3].min() + rng.uniform(0, 3) * h)   # a sheet
        vbi = rng.uniform(1e-5, 4e-5, nb).astype(real)
    if seed % 19 == 18:   # a few particles with NaN / inf coordinates (a caller's bug must not take the device down)
        k = rng.integers(0, n, 5)
        pos[k[:3], int(rng.integers(0, 3))] = np.nan
        pos[k[3:], int(rng.integers(0, 3))] = np.inf
    cfg = {}
    if solver == capi.PBF:   # drawn after every draw of the scene, so that the scenes stay those of the other solvers
        cfg = dict(eta=float(rng.choice([0.0, rng.uniform(0.003, 0.05)])), min_iters=int(rng.integers(1, 5)),
                   relaxation=float(10 ** rng.uniform(-3, -1)), xsph=float(rng.choice([0.0, rng.uniform(0.0, 0.3)])),
                   k=float(rng.choice([0.0, 10 ** rng.uniform(-4, -3)])), dq=float(rng.uniform(0.1, 0.4)),
                   eps_v=float(rng.choice([0.0, rng.uniform(0.0, 1.0)])))
    elif solver == capi.DFSPH:   # (likewise)
        cfg = dict(eta=float(rng.choice([0.0, 10 ** rng.uniform(-4, -2)])), min_iters=int(rng.integers(1, 5)),
                   eta_v=float(rng.choice([0.0, 10 ** rng.uniform(-4, -2)])), min_v=int(rng.integers(0, 4)), warm=int(rng.integers(0, 2)))
    return dict(p=p, n=n, pos=pos, vel=vel, bi=bi, vbi=vbi, solver=solver, double=double, kset=kset, gs=gs, cs=cs, h=h, cfg=cfg,
                dens_mode=int(dens_mode))


def _configure(s, sc):
    c = sc["cfg"]
    if sc["solver"] == capi.PBF:
        s.pbf_configure(c["eta"], c["min_iters"], c["relaxation"], c["xsph"])
        s.pbf_set_tensile(c["k"], c["dq"])
        s.pbf_set_vorticity(c["eps_v"])
    elif sc["solver"] == capi.DFSPH:
        s.dfsph_configure(c["eta"], c["min_iters"], c["eta_v"], c["min_v"], c["warm"])


def _first_difference(seed, sc, names, outs):
    for nm, a, b in zip(names, *outs):
        if not np.array_equal(a, b, equal_nan=True):
            bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
            return "seed %d: %s differs at %d places, first %s (n=%d grid=%s cs/h=%s solver=%d walls=%s double=%s kset=%d cfg=%s)" % (
                seed, nm, len(bad), bad[0], sc["n"], sc["gs"], sc["cs"] / sc["h"], sc["solver"], sc["bi"] is not None, sc["double"],
                sc["kset"], sc["cfg"])
    return None


def one_pci(seed, solver):
    """PCISPH / PBF: production kernels against the reference-order kernels, bit for bit (NaN-aware), at STAGE_P_ADVECT, at
    STAGE_P_SOLVE and after 3 steps (6 on the >= 40,000-particle seeds: the coherent re-sort runs)"""
    sc = make_scene(seed, solver)
    n, pos, vel = sc["n"], sc["pos"], sc["vel"]
    solve = ["sortedPos", "velAdv", "densCorr", "P_l", "forcesP", "posPred"]
    advect = ["sortedPos", "velAdv", "posPred"]
    if solver == capi.DFSPH:   # (no predicted positions; the divergence solve's velocities and Kv, the factor, K)
        solve = ["sortedPos", "velAdv", "densCorr", "P_l", "pres", "dfsphAlpha"]
        advect = ["sortedPos", "sortedVel", "velAdv", "dfsphKappaV"]
    names = ["advect " + x for x in advect] + ["solve " + x for x in solve] + ["iters", "pos", "vel", "pressure"]
    outs = []
    for ref in (False, True):
        s = capi.Solver(sc["p"], n, solver=solver, double=sc["double"], kernel_set=sc["kset"], reference_order=ref)
        _configure(s, sc)
        s.set_particles(pos, vel)
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
        s.step_partial(capi.STAGE_P_ADVECT)
        o = [s.get(x) for x in advect]
        s.set_particles(pos, vel)
        s.step_partial(capi.STAGE_P_SOLVE)
        o += [s.get(x) for x in solve] + [np.array([s.last_iterations])]
        s.set_particles(pos, vel)
        s.step(6 if n >= 40000 else 3)
        o += list(s.download(pressure=True))
        outs.append(o)
        s.close()
    return _first_difference(seed, sc, names, outs)


def one(seed, solver=None):
    if solver in (capi.PCISPH, capi.PBF, capi.DFSPH):
        return one_pci(seed, solver)
    sc = make_scene(seed)
    p, n, pos, vel, bi, vbi, solver, double, kset, gs, cs, h = (sc[k] for k in ("p", "n", "pos", "vel", "bi", "vbi", "solver", "double", "kset", "gs", "cs", "h"))
    outs, iters = [], []
    for ref in (False, True):
        s = capi.Solver(p, n, solver=solver, double=double, kernel_set=kset, reference_order=ref)
        s.set_particles(pos, vel)
        s.set_boundaries(bi, vbi, update_grid=False)
        s.step_partial(capi.STAGE_I_PFORCE if solver == capi.IISPH else capi.STAGE_FORCES)
        o = [s.get("dens"), s.get("forcesP") if solver == capi.IISPH else s.get("forces")]
        iters.append(s.last_iterations if solver == capi.IISPH else 0)
        s.set_particles(pos, vel)
        s.step(6 if n >= 40000 else 3)
        o += list(s.download())
        outs.append(o)
        s.close()
    # A solve that has overflowed (inf pressures in a random clump that does not converge) is not comparable: the list kernels visit
    # only neighbours inside the kernel support, the reference order also multiplies the zero gradients beyond it with the inf
    # (0 * inf = NaN) — equal for finite operands only.
    # (The solver's max(p, 0) clamp can turn such a NaN into a finite 0, so even finite results may then differ: a solve that ran into
    # its iteration cap is skipped as well.)
    if os.environ.get("FUZZ_SKIP_NONFINITE", "0") == "1" and not all(np.isfinite(x).all() for x in outs[1]):
        return "diverged"
    for k, (a, b) in enumerate(zip(*outs)):
        if not np.array_equal(a, b, equal_nan=True):
            bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
            return "seed %d: array %d differs at %d places, first %s (n=%d grid=%s cs/h=%s solver=%d walls=%s double=%s kset=%d)" % (seed, k, len(bad), bad[0], n, gs, cs / h, solver, bi is not None, double, kset)
    return None

# Bars of one_vs_oracle, by precision: fp32 the fixed IISPH tests' 5 x TOL_STAGE; fp64 10 x TOL_STAGE_F64 (tests/test_parity_gpu.py; measured max 7.2e-15)
ORACLE_BARS = {False: 1e-5, True: 1e-12}
ORACLE_OVERFLOW = 1e12   # |P_l| or |sumDij| beyond this (or inf): the oracle's own solve overflowed
IISPH_NAMES = ("dens", "velAdv", "forcesAdv", "diiFluid", "diiBoundary", "densAdv", "aii", "sumDij", "densCorr", "P_l", "pres", "forcesP")


def one_vs_oracle(seed, config=None, errors=None):
    """production kernels against the CPU oracle (tait="double7", the device's Tait convention) on the same random scene, one partial
    step: hash / index bit-exact; SESPH density, pressure and forces, IISPH every intermediate of the chain and the iteration count;
    the non-finite entries equal element for element, the finite ones within ORACLE_BARS of the precision.  Returns None, a failure
    message, or "not comparable" where the oracle's IISPH solve itself overflowed (then roundoff of inf-adjacent values decides, and
    the solver's max(p, 0) can turn a NaN into 0).  `errors`, a dict, collects the largest error per array."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.common import rel_err
    from tests.oracle_lib import IISPH as O_IISPH, SESPH as O_SESPH, STOP_FORCES, STOP_I_PFORCE, Oracle
    sc = make_scene(seed, config=config)
    iis = sc["solver"] == capi.IISPH
    o = Oracle(sc["p"], sc["double"], sc["kset"], O_IISPH if iis else O_SESPH, threads=min(16, os.cpu_count() or 1), tait="double7")
    o.set_particles(sc["pos"], sc["vel"]); o.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    s = capi.Solver(sc["p"], sc["n"], solver=sc["solver"], double=sc["double"], kernel_set=sc["kset"])
    s.set_particles(sc["pos"], sc["vel"]); s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    o.step(1, stop=STOP_I_PFORCE if iis else STOP_FORCES); s.step_partial(capi.STAGE_I_PFORCE if iis else capi.STAGE_FORCES)
    tag = "seed %d vs oracle (n=%d grid=%s solver=%d double=%s kset=%d walls=%s)" % (
        seed, sc["n"], sc["gs"], sc["solver"], sc["double"], sc["kset"], sc["bi"] is not None)
    if iis:
        with np.errstate(invalid="ignore"):
            if any(np.any(np.isinf(x) | (np.abs(x) > ORACLE_OVERFLOW)) for x in (o.get("P_l"), o.get("sumDij"))):
                s.close(); return "not comparable"
    try:
        if not np.array_equal(s.get("hash"), o.get("hash")) or not np.array_equal(s.get("index"), o.get("index")):
            return "%s: hash/index differ" % tag
        if iis and s.last_iterations != o.last_iters:
            return "%s: %d iterations, oracle %d" % (tag, s.last_iterations, o.last_iters)
        for nm in (IISPH_NAMES if iis else ("dens", "pres", "forces")):
            a, b = s.get(nm), o.get(nm)
            fin = np.isfinite(b)
            if not np.array_equal(np.isfinite(a), fin) or not np.array_equal(a[~fin], b[~fin], equal_nan=True):
                return "%s: %s non-finite at %d places, oracle at %d" % (tag, nm, int((~np.isfinite(a)).sum()), int((~fin).sum()))
            e = rel_err(a[fin], b[fin]) if fin.any() else 0.0
            if errors is not None:
                k = (sc["solver"], sc["double"], sc["kset"], nm)
                errors[k] = max(errors.get(k, 0.0), e)
            if not e <= ORACLE_BARS[sc["double"]]:
                return "%s: %s rel %.3g" % (tag, nm, e)
        return None
    finally:
        s.close()


# ---- the SESPH launches selected by flags (NRS_FLAG_STAGED_SCAN, NRS_FLAG_FAST_ARITH) on the soak's scenes -------------------------
FLAGS_CONFIG = dict(solver=capi.SESPH, double=False, kset=1)   # the only solver, precision and kernel set whose plan honours either flag
EXACT_FLAG_SETS = {"staged": capi.FLAG_STAGED_SCAN, "staged+nofusion": capi.FLAG_STAGED_SCAN | capi.FLAG_NO_FUSION,
                   "staged+fullsort": capi.FLAG_STAGED_SCAN | capi.FLAG_FULL_SORT}
FAST_FLAG_SETS = {"fast": capi.FLAG_FAST_ARITH, "fast+staged": capi.FLAG_FAST_ARITH | capi.FLAG_STAGED_SCAN}
FAST_TOL = 1e-5           # the FAST mode's bar, array-relative (tests/test_fast_arith_gpu.py, north-star)
# FAST forces are asserted in every density mode: on the uniform clouds and the jittered lattices (dens_mode 0 and 2) by the mode's
# definition; on the clump scenes (dens_mode 1), where large pair forces cancel, because the measured errors stay within the bar as
# well (largest 7.0e-7 over seeds 9300-9347)
FAST_FORCE_MODES = (0, 1, 2)
FLAGS_TABLES = ("hash", "index", "cellStart", "cellEnd")


def _flags_context(sc, **kw):
    s = capi.Solver(sc["p"], max(sc["n"], 1), solver=capi.SESPH, double=False, kernel_set=1, **kw)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    return s


def _flags_exact_run(sc, **kw):
    """dens / pres at STAGE_DENSITY (the launches without shared lists), the tables and dens / pres / forces at STAGE_FORCES, positions
    and velocities after 3 steps (6 from 40,000 particles: the coherent re-sort runs)"""
    s = _flags_context(sc, **kw)
    s.step_partial(capi.STAGE_DENSITY)
    out = {"density " + k: s.get(k) for k in ("dens", "pres")}
    s.set_particles(sc["pos"], sc["vel"])
    s.step_partial(capi.STAGE_FORCES)
    out.update({k: s.get(k) for k in FLAGS_TABLES + ("dens", "pres", "forces")})
    s.set_particles(sc["pos"], sc["vel"])
    s.step(6 if sc["n"] >= 40000 else 3)
    out["pos"], out["vel"] = s.download()
    s.close()
    return out


def flags_reference(seed, shared=None, oracle=False):
    """What one_flags compares with, computed once per seed when the caller keeps `shared` (a dict): the scene under FLAGS_CONFIG, the
    reference-order context's run of it and, with oracle=True, the CPU oracle's density and forces (fp32, tait="double7", as
    one_vs_oracle runs it)."""
    shared = {} if shared is None else shared
    ent = shared.setdefault(seed, {})
    if "sc" not in ent:
        ent["sc"] = make_scene(seed, config=FLAGS_CONFIG)
        ent["ref"] = _flags_exact_run(ent["sc"], reference_order=True)
        # (the cell tables of 48 cached seeds, up to 2^27 cells each, would not fit: the non-empty cells only)
        cs, ce = ent["ref"].pop("cellStart"), ent["ref"].pop("cellEnd")
        full = np.flatnonzero(cs != 0xFFFFFFFF)
        ent["cells"] = (len(cs), full, cs[full], ce[full])
    if oracle and "oracle" not in ent:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from tests.oracle_lib import SESPH as O_SESPH, STOP_FORCES, Oracle
        sc = ent["sc"]
        o = Oracle(sc["p"], False, 1, O_SESPH, threads=min(16, os.cpu_count() or 1), tait="double7")
        o.set_particles(sc["pos"], sc["vel"]); o.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
        o.step(1, stop=STOP_FORCES)
        ent["oracle"] = {k: o.get(k) for k in ("dens", "forces")}
    return ent


def one_flags(seed, flags, shared=None, errors=None):
    """The seed's scene as fp32 Muller SESPH (FLAGS_CONFIG; every other draw is the seed's own) in a context with `flags`.
    Without NRS_FLAG_FAST_ARITH: everything _flags_exact_run reads equals the reference-order context's bit for bit (NaN-aware).
    With it: hash, index and the cell tables equal the reference-order context's bit for bit; after one STAGE_FORCES (NRS_FLAG_NO_FUSION
    added) density and forces against the CPU ORACLE through close_masked — the non-finite entries element for element, the finite
    ones within FAST_TOL: density on every seed, forces where the scene's dens_mode is in FAST_FORCE_MODES (all three).  One step
    only: afterwards the output order of the two arithmetics diverges (tests/test_fast_arith_gpu.py).  Returns None or a failure
    message; `errors`, a dict, collects the error of each quantity as errors[(seed, dens_mode, "dens" | "forces")]."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.common import check_cell_tables, close_masked
    fast = bool(flags & capi.FLAG_FAST_ARITH)
    ent = flags_reference(seed, shared, oracle=fast)
    sc, ref = ent["sc"], ent["ref"]
    ncells, full, cs_full, ce_full = ent["cells"]
    ref_cs, ref_ce = np.full(ncells, 0xFFFFFFFF, np.uint32), np.zeros(ncells, np.uint32)
    ref_cs[full], ref_ce[full] = cs_full, ce_full
    tag = "seed %d flags %d (n=%d grid=%s cs/h=%s walls=%s dens_mode=%d)" % (seed, flags, sc["n"], sc["gs"], sc["cs"] / sc["h"],
                                                                             sc["bi"] is not None, sc["dens_mode"])
    if not fast:
        got = _flags_exact_run(sc, flags=flags)
        for k in ref:
            if not np.array_equal(got[k], ref[k], equal_nan=True):
                bad = np.argwhere(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))
                return "%s: %s differs at %d places, first %s" % (tag, k, len(bad), bad[0])
        try:
            check_cell_tables(got["cellStart"], got["cellEnd"], ref_cs, ref_ce)
        except AssertionError as e:
            return "%s: cell tables differ: %s" % (tag, str(e)[:200])
        return None
    s = _flags_context(sc, flags=flags | capi.FLAG_NO_FUSION)
    s.step_partial(capi.STAGE_FORCES)
    got = {k: s.get(k) for k in FLAGS_TABLES + ("dens", "forces")}
    s.close()
    try:
        np.testing.assert_array_equal(got["hash"], ref["hash"], err_msg="hash")
        np.testing.assert_array_equal(got["index"], ref["index"], err_msg="index")
        check_cell_tables(got["cellStart"], got["cellEnd"], ref_cs, ref_ce)
        for nm in ("dens", "forces"):
            asserted = nm == "dens" or sc["dens_mode"] in FAST_FORCE_MODES
            e = close_masked(got[nm], ent["oracle"][nm], FAST_TOL if asserted else np.inf, "%s %s" % (tag, nm))
            if errors is not None:
                errors[(seed, sc["dens_mode"], nm)] = e
    except AssertionError as e:
        return "%s: %s" % (tag, str(e)[:300])
    return None


MODEL_DENSITY = (1.2, 1.5)
# The Monaghan kernels do not vanish at the loop's cut-off h: W(h) = 1 / (4 pi h^3) and grad W(h) != 0, so a pair whose length lies
# within the roundoff of the two computations from h enters one sum and not the other, a whole term apart (4 % of rho for one pair).
# The model takes the device's own start state and forms the first iteration's separations in the build's precision, so its cut-off
# decisions up to there are the device's; after that (PBF's XSPH launch at the corrected positions) a Monaghan scene with a pair
# within MONAGHAN_CUT_MARGIN of h is not comparable.  Muller's W and gradient vanish at h.
MONAGHAN_CUT_MARGIN = 1e-5


def make_model_scene(seed, solver):
    """make_scene(seed, solver) cut down for the float64 models (brute-force pairs): the 300-2,500 particles and at most 1,500 wall
    particles nearest to one particle of the cloud, and only geometry where the device's candidate rule is "every pair within h,
    once" — the rule the models apply:
      * every cell edge >= h (a cell edge below h misses pairs: the walk covers one cell each way),
      * every grid axis >= 4 cells (an axis of 1-2 cells makes the 27-cell walk visit a cell twice, counting its pairs twice);
    far origins, grids that wrap and wall sheets stay.  The NaN / inf coordinates are dropped: a model result with them is not finite.
    One fixed iteration: after a correction, rho* / rho0 - 1 of the few corrected particles of a random piece is the loop's residual,
    and its roundoff (fp32; and the float length() of fp64) reached 3e-3 of max |lambda| with 1-3 iterations on 12 of 400 seeds.  The
    fixed scenes of tests/test_pcisph_gpu.py and tests/test_pbf_gpu.py, compressed throughout, run 3 iterations.
    The grid keeps its cells and origin; the piece may be scaled (below), so it may lie partly outside the grid and wrap."""
    sc = make_scene(seed, solver)
    rng = np.random.default_rng(seed + 1_000_003)
    real = np.float64 if sc["double"] else np.float32
    p, h = sc["p"], sc["h"]
    pos = sc["pos"][np.all(np.isfinite(sc["pos"]), axis=1)]
    c = pos[int(rng.integers(0, len(pos))), :3]   # the particles nearest to one of them: a piece of the cloud at its own density
    pos = pos[np.argsort(np.linalg.norm(pos[:, :3] - c, axis=1), kind="stable")[:int(rng.integers(300, 2500))]]
    # A clump of the soak holds up to ~60x rest density: its first iteration throws particles metres apart, what the next one finds
    # within h is chance, and fp32 roundoff of such a state is far above the bars; a piece just above rest density leaves C =
    # rho / rho0 - 1 at the level of fp32 roundoff.  So the piece is scaled about c until its maximum start density (fluid only, the
    # scene's kernel set) lies in MODEL_DENSITY x rho0 — the compression of the fixed model scenes.
    from tests.pcisph_model import W, pairs_within
    m, rd = float(p["particleMass"][0]), float(p["restDensity"][0])
    lo_, hi_ = MODEL_DENSITY
    for _ in range(12):
        i, j = pairs_within(pos, pos, h, same=True)
        rho = m * W(p, np.zeros((1, 3)), sc["kset"])[0] + np.bincount(i, m * W(p, pos[i, :3] - pos[j, :3], sc["kset"]), len(pos))
        if lo_ * rd <= rho.max() <= hi_ * rd:
            break
        f = np.clip(np.cbrt(rho.max() / (0.5 * (lo_ + hi_) * rd)), 0.8, 4.0)
        pos[:, :3] = (c + (pos[:, :3].astype(np.float64) - c) * f).astype(real)
    cs = np.maximum(sc["cs"], h)
    p["cellSize"][0] = cs.astype(real)
    gs = [max(4, g) for g in sc["gs"]]
    while gs[0] * gs[1] * gs[2] > 2 ** 27: gs[int(np.argmax(gs))] //= 2
    p["gridSize"][0] = gs; p["numCells"][0] = gs[0] * gs[1] * gs[2]
    bi, vbi = sc["bi"], sc["vbi"]
    if bi is not None and len(bi) > 1500:
        k = np.argsort(np.linalg.norm(bi[:, :3] - c, axis=1), kind="stable")[:1500]
        bi, vbi = bi[k], vbi[k]
    cfg = dict(sc["cfg"], eps_v=0.0)   # (confinement: whether N is set is decided by roundoff near its cut, tests/test_pbf_extras_gpu.py)
    return dict(sc, p=p, n=len(pos), pos=pos, vel=sc["vel"][:len(pos)], bi=bi, vbi=vbi, gs=gs, cs=cs, cfg=cfg,
                iters=1, ref=bool(rng.integers(0, 2)))


def one_dfsph_vs_model(seed):
    """DFSPH: the device against tests/dfsph_model.py on make_model_scene, moving (the scene's velocities): one fixed iteration per loop
    (the divergence solve on or off and the warm start as drawn; from an upload K_prev = Kv_prev = 0), both paths, with the bars of the
    model tests.  Inputs are the device's sorted state after DENSITY and its vel_adv after P_ADVECT."""
    from tests import dfsph_model
    from tests.common import rel_err
    sc = make_model_scene(seed, capi.DFSPH)
    p, c = sc["p"], sc["cfg"]
    tol = 1e-10 if sc["double"] else 1e-4
    mn_v = min(c["min_v"], 1)
    s = capi.Solver(p, max(sc["n"], 1), solver=capi.DFSPH, double=sc["double"], kernel_set=sc["kset"], reference_order=sc["ref"])
    s.dfsph_configure(0.0, 1, 0.0, mn_v, c["warm"])
    dev = {}
    for stage, names in ((capi.STAGE_DENSITY, ("sortedPos", "sortedVel", "dens", "dfsphAlpha")), (capi.STAGE_P_ADVECT, ("sortedVel", "velAdv")),
                         (capi.STAGE_P_SOLVE, ("velAdv", "pres", "P_l", "densCorr"))):
        s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
        s.step_partial(stage)
        dev.update({"%d %s" % (stage, nm): s.get(nm) for nm in names})
    bs = s.get("bSorted") if sc["bi"] is not None else None
    s.close()
    x, v0 = dev["4 sortedPos"], dev["4 sortedVel"]
    pairs = dfsph_model.Pairs(p, x, None if bs is None else bs[:, :3], None if bs is None else bs[:, 3], sc["kset"])
    alpha, _ = dfsph_model.factor(p, pairs, sc["kset"])
    fields = [("alpha", dev["4 dfsphAlpha"], alpha)]
    if mn_v:
        div = dfsph_model.solve(p, pairs, alpha, v0, min_iters=1, warm=bool(c["warm"]))
        fields.append(("v_df", dev["7 sortedVel"], div["u"]))
    den = dfsph_model.solve(p, pairs, alpha, dev["7 velAdv"], rho=dev["4 dens"], min_iters=1, warm=bool(c["warm"]))
    fields += [("vstar", dev["8 velAdv"], den["u"]), ("K", dev["8 pres"], den["K"]), ("kappa", dev["8 P_l"], den["kappa"]),
               ("rho_adv", dev["8 densCorr"], den["rho_adv"])]
    if not all(np.all(np.isfinite(w)) for _, _, w in fields):
        return "not comparable"
    tag = "seed %d dfsph vs model (n=%d grid=%s cs/h=%s walls=%s double=%s kset=%d ref=%s cfg=%s)" % (
        seed, sc["n"], sc["gs"], sc["cs"] / sc["h"], sc["bi"] is not None, sc["double"], sc["kset"], sc["ref"], c)
    for nm, got, want in fields:
        got = got[:, :3] if want.ndim == 2 else got
        if not rel_err(got, want) <= tol:
            return "%s: %s rel %.3g" % (tag, nm, rel_err(got, want))
    return None


def one_vs_model(seed, solver):
    """the device against the float64 model (tests/pcisph_model.py, tests/pbf_extras_model.py) on make_model_scene: one fixed
    iteration, both paths, both precisions and kernel sets by seed, with the bars of the model tests (rel. 1e-4 fp32, 1e-10 fp64;
    PBF velocities 10x).  Returns None, a failure message, "not comparable" where the model's own result is not finite, or "near cut"
    for a Monaghan scene with a pair within MONAGHAN_CUT_MARGIN of h where the model's positions are no longer the device's."""
    if solver == capi.DFSPH:
        return one_dfsph_vs_model(seed)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import pbf_extras_model, pcisph_model
    from tests.common import rel_err
    sc = make_model_scene(seed, solver)
    p, L, c = sc["p"], sc["iters"], sc["cfg"]
    tol = 1e-10 if sc["double"] else 1e-4
    s = capi.Solver(p, max(sc["n"], 1), solver=solver, double=sc["double"], kernel_set=sc["kset"], reference_order=sc["ref"])
    if solver == capi.PCISPH:
        s.pcisph_configure(0.01, L)
        s.set_max_iterations(L)
    else:
        _configure(s, dict(sc, cfg=dict(c, eta=0.0, min_iters=L)))
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, va = s.get("sortedPos"), s.get("velAdv")
    bs = s.get("bSorted") if sc["bi"] is not None else None
    s.set_particles(sc["pos"], sc["vel"])
    s.step_partial(capi.STAGE_P_SOLVE)
    dev = {nm: s.get(nm) for nm in ("densCorr", "P_l", "forcesP", "posPred")}
    iters = s.last_iterations
    stat = s.get_stat(capi.STAT_PCISPH_DELTA if solver == capi.PCISPH else capi.STAT_PBF_EPSILON)
    s.set_particles(sc["pos"], sc["vel"])
    s.step(1)
    dpos, dvel, dpres = s.download(pressure=True)
    s.close()
    bpos, vb = (None, None) if bs is None else (bs[:, :3], bs[:, 3])
    if solver == capi.PCISPH:
        want = pcisph_model.prototype_delta(p, kernel_set=sc["kset"])[0]
        m = pcisph_model.run(p, x, va, bpos, vb, delta=stat, min_iters=L, cap=L, kernel_set=sc["kset"])
        fields = (("densCorr", m["rho"]), ("P_l", m["p"]), ("forcesP", m["fp"]), ("posPred", m["xs"]))
        final = (("pos", dpos, m["pos"], tol), ("vel", dvel, m["vel"], tol), ("pressure", dpres, m["p"], tol))
    else:
        want = c["relaxation"] * pbf_extras_model.prototype_d(p, sc["kset"])[0]
        m = pbf_extras_model.run(p, x, va, bpos, vb, eps=stat, min_iters=L, eta=0.0, xsph=c["xsph"], k=c["k"], dq=c["dq"],
                                 kernel_set=sc["kset"])
        fields = (("densCorr", m["rho"]), ("P_l", m["lam"]), ("forcesP", m["dx"]), ("posPred", m["xs"]))
        final = (("pos", dpos, m["pos"], tol), ("vel", dvel, m["vel"], 10 * tol), ("pressure", dpres, m["lam"], tol))
    if not all(np.all(np.isfinite(v)) for _, v in fields):
        return "not comparable"
    if sc["kset"] == capi.MONAGHAN and m["margin"] < MONAGHAN_CUT_MARGIN:
        return "near cut"
    tag = "seed %d vs model (n=%d grid=%s cs/h=%s solver=%d walls=%s double=%s kset=%d ref=%s iters=%d cfg=%s)" % (
        seed, sc["n"], sc["gs"], sc["cs"] / sc["h"], solver, sc["bi"] is not None, sc["double"], sc["kset"], sc["ref"], L, c)
    if iters != L:
        return "%s: %d iterations" % (tag, iters)
    if not abs(stat / want - 1) <= 1e-5:
        return "%s: prototype %r, model %r" % (tag, stat, want)
    for nm, want in fields:
        got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
        if not rel_err(got, want) <= tol:
            return "%s: %s rel %.3g" % (tag, nm, rel_err(got, want))
    for nm, got, want, t in final:
        got = got[:, :3] if want.ndim == 2 else got
        if not rel_err(got, want) <= t:
            return "%s: %s rel %.3g" % (tag, nm, rel_err(got, want))
    return None


# ---- the read-out side (sampler, surface, anisotropic passes, diffuse particles, attribute diffusion) on pieces of the soak's scenes ----
READER_MODES = ("sample", "surface", "aniso", "diffuse", "track")
READER_MAX_NODES = 16384


def make_reader_scene(seed, min_axis=4, max_particles=None):
    """make_scene(seed, SESPH) cut down for the models of the readers (brute-force pairs), as make_model_scene cuts it, with draws of
    its own (default_rng(seed + 2_000_003)): the K in 300..1500 particles nearest to one finite particle of the cloud (stable argsort)
    with their velocities, the at most 1,500 wall particles nearest to it, cellSize = max(cs, h) per axis and every grid axis
    max(min_axis, g) — the geometry sample_refusal accepts (8 cells for the anisotropic passes).  The origin stays, far ones included,
    and so does the wrap.  Unlike make_model_scene the piece is NOT rescaled (the readers solve nothing: a clump at 60 x rest density
    is what they should meet), and on the seed % 19 == 18 scenes the scene's NaN / inf rows are put back behind the piece.
    max_particles: a cap on the whole piece (the anisotropic model holds N x N arrays)."""
    sc = make_scene(seed, capi.SESPH)
    rng = np.random.default_rng(seed + 2_000_003)
    real = np.float64 if sc["double"] else np.float32
    p, h = sc["p"], sc["h"]
    fin = np.all(np.isfinite(sc["pos"]), axis=1)
    good, bad = np.flatnonzero(fin), np.flatnonzero(~fin)
    c = sc["pos"][good[int(rng.integers(0, len(good)))], :3]
    k = int(rng.integers(300, 1501))
    if max_particles:
        k = min(k, max_particles - len(bad))
    near = good[np.argsort(np.linalg.norm(sc["pos"][good, :3] - c, axis=1), kind="stable")[:k]]
    keep = np.concatenate([near, bad])
    pos, vel = sc["pos"][keep].copy(), sc["vel"][keep].copy()
    cs = np.maximum(sc["cs"], h)
    p["cellSize"][0] = cs.astype(real)
    gs = [max(min_axis, g) for g in sc["gs"]]
    while gs[0] * gs[1] * gs[2] > 2 ** 27: gs[int(np.argmax(gs))] //= 2
    p["gridSize"][0] = gs; p["numCells"][0] = gs[0] * gs[1] * gs[2]
    bi, vbi = sc["bi"], sc["vbi"]
    if bi is not None and len(bi) > 1500:
        kb = np.argsort(np.linalg.norm(bi[:, :3] - c, axis=1), kind="stable")[:1500]
        bi, vbi = bi[kb], vbi[kb]
    return dict(sc, seed=seed, p=p, n=len(pos), pos=pos, vel=vel, bi=bi, vbi=vbi, gs=gs, cs=cs, nonfinite=len(bad), real=real)


def reader_box(sc):
    """the bounding box of the piece's finite particles, float64"""
    x = sc["pos"][np.all(np.isfinite(sc["pos"]), axis=1), :3].astype(np.float64)
    return x.min(0), x.max(0)


def reader_lattice(sc, pad=2.0):
    """(origin, spacing, dims): the piece's box inflated by pad * h at the smallest spacing from h / 2 up (steps of 10 %) that keeps the
    lattice at or below READER_MAX_NODES nodes; with pad >= 2 every border node is farther than h from every particle"""
    lo, hi = reader_box(sc)
    lo, hi = lo - pad * sc["h"], hi + pad * sc["h"]
    sp = sc["h"] / 2
    while True:
        dims = tuple(int(np.ceil((hi[a] - lo[a]) / sp)) + 1 for a in range(3))
        if dims[0] * dims[1] * dims[2] <= READER_MAX_NODES:
            return tuple(float(v) for v in lo), float(sp), dims
        sp *= 1.1


def reader_queries(sc, attempt=0, m=700):
    """The query set of one_sample, (m, 4) in the scene's precision, m no multiple of 64: rows 0-39 particle positions bit for bit,
    40-79 points near particles moved by whole grid extents to beyond the grid's box (their cells wrap; the axis cycles x, y, z, the
    side alternates every three), 80 / 81 at +-1e30 (saturated cell coordinates), 82 with a NaN, 83 with an inf coordinate, 84-143
    near wall particles where the scene has walls, the rest uniform in the piece's box +- 2 h.  attempt: another draw, for a set with
    a dropped pair (reader_queries_checked).
    Rows 40-79 show only that a wrapped cell yields no false hit: the particles their cells alias to are whole grid extents away, so
    the count is 0 on both sides.  Sums ACROSS the wrap come from the scenes whose particles lie outside the grid box, through the
    uniform rows and rows 0-39."""
    rng = np.random.default_rng([sc["seed"], 3_000_017, attempt])
    real, h, p = sc["real"], sc["h"], sc["p"]
    fin = sc["pos"][np.all(np.isfinite(sc["pos"]), axis=1)]
    lo, hi = reader_box(sc)
    q = np.ones((m, 4), real)
    q[:, :3] = rng.uniform(lo - 2 * h, hi + 2 * h, (m, 3)).astype(real)
    q[:40] = fin[rng.integers(0, len(fin), 40)]
    q[:40, 3] = 1
    wo = np.asarray(p["worldOrigin"][0], np.float64)
    ext = np.asarray(sc["gs"], np.float64) * np.asarray(p["cellSize"][0], np.float64)
    base = fin[rng.integers(0, len(fin), 40), :3].astype(np.float64) + rng.uniform(-0.3 * h, 0.3 * h, (40, 3))
    for t in range(40):
        a, up = t % 3, (t // 3) % 2
        x = base[t].copy()
        if up:
            x[a] += ext[a] * max(np.floor((wo[a] + ext[a] - x[a]) / ext[a]) + 1, 0)
        else:
            x[a] -= ext[a] * max(np.floor((x[a] - wo[a]) / ext[a]) + 1, 0)
        q[40 + t, :3] = x.astype(real)
    q[80, :3], q[81, :3] = 1e30, -1e30
    q[82, 1], q[83, 0] = np.nan, np.inf
    if sc["bi"] is not None:   # the nearest wall particles of most pieces lie outside the piece's box: 60 queries within 0.6 h of some
        q[84:144, :3] = (sc["bi"][rng.integers(0, len(sc["bi"]), 60), :3].astype(np.float64) + rng.uniform(-0.6 * h, 0.6 * h, (60, 3))).astype(real)
    assert m % 64 != 0
    return q


def reader_dropped(sc, owners, reach=1, radius=None, squared=False, same=False, walls=True):
    """diffuse_model.dropped_pairs of `owners` against the piece's particles and (walls) its wall particles"""
    from tests import diffuse_model as dm
    n = dm.dropped_pairs(sc["p"], owners, sc["pos"], sc["real"], radius, reach, squared, same)
    if walls and sc["bi"] is not None:
        n += dm.dropped_pairs(sc["p"], owners, sc["bi"], sc["real"], radius, reach, squared)
    return n


def reader_queries_checked(sc, attempts=8):
    """(queries, attempt): the first draw of reader_queries without a dropped pair (a set with one is replaced, not skipped)"""
    for attempt in range(attempts):
        q = reader_queries(sc, attempt)
        if reader_dropped(sc, q[np.all(np.isfinite(q[:, :3]), axis=1)]) == 0:
            return q, attempt
    raise AssertionError("seed %d: every one of %d query sets has a pair beyond the walk's reach" % (sc["seed"], attempts))


def reader_diffuse_config(sc, capacity=1 << 20):
    """the diffuse settings of a piece: SETTINGS of tests/test_diffuse_model_cpu.py with spray_below / bubble_above at the 33 % and 66 %
    quantiles of the piece's neighbour counts (the particle included, as the kinds count): with the dam's 5 / 6 a dense piece gives
    only bubbles"""
    from tests import diffuse_model as dm
    from tests.test_diffuse_model_cpu import SETTINGS
    i, _, _ = dm.walk_pairs(sc["p"], sc["pos"], sc["pos"], sc["real"], same=True)
    cnt = 1 + np.bincount(i, minlength=sc["n"])[np.all(np.isfinite(sc["pos"]), axis=1)]
    lo_, hi_ = int(np.quantile(cnt, 0.33)), int(np.quantile(cnt, 0.66))
    return dm.config(**dict(SETTINGS, capacity=capacity, spray_below=lo_, bubble_above=max(hi_, lo_)))


READER_DIFFUSE_STEPS = 3


def reader_moved(params, pos, vel, real):
    """pos + dt * vel in the build's precision, dt the parameters' timestep: the fluid one upload on"""
    out = pos.copy()
    with np.errstate(invalid="ignore"):
        out[:, :3] = pos[:, :3] + real(params["timestep"][0]) * vel[:, :3]
    return out


def reader_diffuse_run(sc, params=None, pos=None, vel=None):
    """The model's run of one_diffuse: READER_DIFFUSE_STEPS diffuse steps of tests/diffuse_model.py from an empty set, the fluid moved
    by pos + dt * vel between them.  Odd seeds run with a capacity of half the total of the model's own unbounded run (where that is
    above 1).  Returns (cfg, capacity or None, fluid states, step results)."""
    from tests import diffuse_model as dm
    params = sc["p"] if params is None else params
    pos, vel = (sc["pos"] if pos is None else pos), (sc["vel"] if vel is None else vel)
    real = sc["real"]
    cfg = reader_diffuse_config(sc)
    states = [pos]
    for _ in range(READER_DIFFUSE_STEPS - 1):
        states.append(reader_moved(params, states[-1], vel, real))

    def run(cap):
        dpos, dvel, out = np.zeros((0, 4), real), np.zeros((0, 4), real), []
        for k in range(READER_DIFFUSE_STEPS):
            r = dm.step(params, cfg, states[k], vel, dpos, dvel, k, 0.0, sc["kset"], cap)
            dpos, dvel = r["pos"], r["vel"]
            out.append(r)
        return out
    res, cap = run(None), None
    if sc["seed"] % 2 == 1 and res[-1]["total"] // 2 >= 1:
        cap = res[-1]["total"] // 2
        res = run(cap)
    return cfg, cap, states, res


def _reader_context(sc):
    s = capi.Solver(sc["p"], max(sc["n"], 1), solver=capi.SESPH, double=sc["double"], kernel_set=sc["kset"])
    s.set_particles(sc["pos"], sc["vel"])
    if sc["bi"] is not None:
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    return s


def _reader_tag(sc, what):
    return "seed %d %s (n=%d grid=%s cs/h=%s walls=%s double=%s kset=%d nonfinite=%d)" % (
        sc["seed"], what, sc["n"], sc["gs"], sc["cs"] / sc["h"], sc["bi"] is not None, sc["double"], sc["kset"], sc["nonfinite"])


def _reader_guard(fn):
    """(seed, errors=None) -> None | failure text: an AssertionError or a refusal of the library becomes the text"""
    def run(seed, errors=None):
        try:
            return fn(seed, {} if errors is None else errors)
        except (AssertionError, capi.NereusError) as e:
            return "seed %d %s: %s" % (seed, fn.__name__, str(e)[:400])
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


def _ratio(err, bound, sel=None):
    sel = (bound > 0) if sel is None else (sel & (bound > 0))
    return float((err[sel] / bound[sel]).max()) if sel.any() else 0.0


@_reader_guard
def one_sample(seed, errors):
    """nrs_sample_points on reader_queries, all four outputs, without and with FIELD_WALLS, against tests/sample_model.py through its
    compare (counts exact, the rest within the derived bound); the +-1e30 and non-finite queries give zeros; nrs_sample_lattice on
    reader_lattice byte-equal to nrs_sample_points on its nodes.  errors[seed]: max(error / bound) per field."""
    from tests import sample_model as sm
    sc = make_reader_scene(seed)
    q, attempt = reader_queries_checked(sc)
    tag = _reader_tag(sc, "sample")
    out = [capi.FIELD_DENSITY, capi.FIELD_GRADIENT, capi.FIELD_VELOCITY, capi.FIELD_COUNT]
    s = _reader_context(sc)
    try:
        pos, vel = s.download()
        assert pos.tobytes() == sc["pos"].tobytes() and vel.tobytes() == sc["vel"].tobytes(), tag + ": the upload came back changed"
        bs = s.get("bSorted") if sc["bi"] is not None else None
        worst = {}
        for walls in (0, capi.FIELD_WALLS):
            s.sample_points(q, sum(out) | walls)
            got = {f: s.sample_result(f) for f in out}
            want = sm.sample(s.params, pos, vel, q, sc["kset"], bs if walls else None)
            for k, v in sm.compare(got, want, "%s walls=%d" % (tag, walls)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            for f in out:   # saturated cell coordinates, NaN, inf: zeros, count 0
                assert not got[f][80:84].any(), (tag, "a query at +-1e30 or a non-finite one has a result", f)
        origin, sp, dims = reader_lattice(sc)
        nodes = sm.lattice_points(origin, sp, dims, sc["real"])
        for walls in (0, capi.FIELD_WALLS):
            s.sample_lattice(origin, sp, dims, sum(out) | walls)
            a = {f: s.sample_result(f) for f in out}
            s.sample_points(nodes, sum(out) | walls)
            for f in out:
                assert a[f].tobytes() == s.sample_result(f).tobytes(), (tag, "lattice and points differ in field %d, walls=%d" % (f, walls))
        errors[seed] = dict(worst, query_attempt=attempt)
    finally:
        s.close()
    return None


def reader_surface_walls(seed):
    """whether one_surface sets SURFACE_WALLS: every second seed, the EVEN ones — 9416 and 9422, the two scenes of the committed slice
    whose wall sheet reaches the piece's lattice, are among them (tests/test_readers_fuzz_cpu.py asserts that the wall term changes
    the inside mask there)"""
    return seed % 2 == 0


def reader_wall_nodes(sc, origin, sp, dims):
    """bool per lattice node: some wall particle lies within h (float length of the difference in the scene's precision)"""
    from tests import pcisph_model as pm
    from tests.sample_model import lattice_points
    sees = np.zeros(dims[0] * dims[1] * dims[2], bool)
    if sc["bi"] is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            i, _ = pm.pairs_within(lattice_points(origin, sp, dims, sc["real"])[:, :3], sc["bi"][:, :3].astype(sc["real"]), sc["h"], real=sc["real"])
        sees[i] = True
    return sees


@_reader_guard
def one_surface(seed, errors):
    """nrs_surface_extract on reader_lattice at iso = 0.5 rho0 with both attributes, every second seed (reader_surface_walls) with
    SURFACE_WALLS, through tests/test_surface_gpu.py extract_and_check: bit for bit surface_model.extract on the sampler's arrays, and
    mesh_checks — closed unless the wall term reaches a border node of the lattice.  With the flag, the meshed density equals the
    wall-less one at the nodes that see no wall particle and exceeds it at most of those that do.  errors[seed]: V, T, nodes that see a wall."""
    from tests.test_surface_gpu import ATTRS, extract_and_check
    sc = make_reader_scene(seed)
    walls = reader_surface_walls(seed)
    origin, sp, dims = reader_lattice(sc)
    sees = reader_wall_nodes(sc, origin, sp, dims) if walls else np.zeros(int(np.prod(dims)), bool)
    border = np.ones(dims[::-1], bool)
    border[1:-1, 1:-1, 1:-1] = False
    s = _reader_context(sc)
    try:
        flags = ATTRS | (capi.SURFACE_WALLS if walls else 0)
        tag = _reader_tag(sc, "surface")
        m, want, dens = extract_and_check(s, origin, sp, dims, 0.5 * float(sc["p"]["restDensity"][0]), flags, not sees[border.ravel()].any(), tag)
        if walls:
            s.sample_lattice(origin, sp, dims, capi.FIELD_DENSITY)
            plain = s.sample_result(capi.FIELD_DENSITY)
            assert np.array_equal(dens[~sees], plain[~sees]) and np.all(dens[sees] >= plain[sees]), tag + ": the wall term away from the walls"
            # (a wall particle at almost h adds a term that may round away: most of the nodes that see one, not all)
            assert sees.sum() < 10 or (dens > plain).sum() > sees.sum() // 2, tag + ": the wall term is missing from the meshed density"
        errors[seed] = dict(V=int(want["V"]), T=int(want["T"]), nodes=int(np.prod(dims)), wall_nodes=int(sees.sum()),
                            wall_changed=int((dens > plain).sum()) if walls else 0)
    finally:
        s.close()
    return None


ANISO_MAX_PARTICLES = 1200


@_reader_guard
def one_aniso(seed, errors):
    """The anisotropic passes on make_reader_scene(seed, min_axis=8) of at most ANISO_MAX_PARTICLES particles.  Pass A against
    aniso_model.records: count, index and the liveness masks exact, centre / weight / G / bound within RECORD_CAP of
    tests/test_aniso_gpu.py (the cap that marks a defect; the dam's measured maxima do not transfer to clumps).  The extract bit for
    bit surface_model.extract on sample_result(DENSITY), closed; pass B on that lattice against aniso_model.field from the device's own
    records within its a-priori bound.  errors[seed]: the record errors and max(error / bound) of phi, gradient, velocity."""
    from tests import aniso_model as am
    from tests.test_aniso_gpu import ATTRS, RECORD_CAP, compare_field, extract_and_check, records
    sc = make_reader_scene(seed, min_axis=8, max_particles=ANISO_MAX_PARTICLES)
    tag = _reader_tag(sc, "aniso")
    real, h = sc["real"], float(sc["p"]["interactionRadius"][0])
    r2h = float(real(2) * real(h))
    assert reader_dropped(sc, sc["pos"], reach=2, radius=r2h, squared=True, same=True, walls=False) == 0, tag + ": a pair within 2 h beyond the walk's reach"
    origin, sp, dims = reader_lattice(sc, pad=2.5)
    from tests.sample_model import lattice_points
    assert reader_dropped(sc, lattice_points(origin, sp, dims, real), reach=2, radius=2.0001 * h, walls=False) == 0, tag + ": a node within 2 h beyond the walk's reach"
    s = _reader_context(sc)
    try:
        pos, vel = s.download()
        s.aniso_build(None)
        c, b, g, w, count, index = records(s)
        n = len(pos)
        assert len(count) == n and np.array_equal(np.sort(index), np.arange(n)), tag + " index"
        want = am.records(pos, h, real)
        np.testing.assert_array_equal(count, want["count"][index], err_msg=tag + " count")
        live = want["weight"][index] > 0
        assert np.array_equal(w > 0, live) and np.array_equal(b > 0, live), tag + " liveness"
        support = am.config(h)["support"]
        e = dict(center=0.0, weight=0.0, bound=0.0, G=float(np.linalg.norm(g - want["G"][index], axis=(1, 2)).max() * support))
        if live.any():
            e.update(center=float(np.abs(c[live] - want["center"][index][live]).max() / h),
                     weight=float(np.abs(w[live] / want["weight"][index][live] - 1).max()),
                     bound=float(np.abs(b[live] / want["bound"][index][live] - 1).max()))
        print("%s: centre / h %.3g, weight (relative) %.3g, bound (relative) %.3g, |G - G_model|_F support %.3g" % (tag, e["center"], e["weight"], e["bound"], e["G"]))
        errors[seed] = dict(e)
        cap = RECORD_CAP[64 if sc["double"] else 32]
        for k, v in e.items():
            assert v <= cap, (tag, k, v, "above the cap: a defect, not a tolerance")
        extract_and_check(s, origin, sp, dims, 0.5, ATTRS, True, tag)
        index = s.aniso_result(capi.ANISO_INDEX)
        fw, fg = compare_field(s, origin, sp, dims, vel[index], tag)
        errors[seed].update(phi=_ratio(np.abs(fg["phi"] - fw["phi"]), fw["phi_bound"]),
                            grad=_ratio(np.abs(fg["grad"][:, :3] - fw["grad"]), fw["grad_bound"]),
                            vel=_ratio(np.abs(fg["vel"] - fw["vel"]), fw["vel_bound"], fw["vel_checked"][:, None] & np.ones((1, 4), bool)))
    finally:
        s.close()
    return None


@_reader_guard
def one_diffuse(seed, errors):
    """READER_DIFFUSE_STEPS nrs_diffuse_steps in lockstep with tests/diffuse_model.py (reader_diffuse_run) through
    tests/test_diffuse_gpu.py check_step: normals, potentials, births, kinds, positions, lifetimes, velocities, counts and `dropped`
    byte for byte; the fluid is moved by upload between the steps.  errors[seed]: the totals of the run."""
    from tests.test_diffuse_gpu import check_step
    sc = make_reader_scene(seed)
    tag = _reader_tag(sc, "diffuse")
    s = _reader_context(sc)
    try:
        pos, vel = s.download()
        cfg, cap, states, res = reader_diffuse_run(sc, s.params, pos, vel)
        s.diffuse_configure(**dict(cfg, capacity=cap or (1 << 15)))
        assert res[-1]["total"] <= (1 << 15) or cap, tag
        dropped = 0
        for k, r in enumerate(res):
            if k:
                s.set_particles(states[k], vel)
            s.diffuse_step()
            dropped += r["dropped"]
            check_step(s, r, "%s step %d" % (tag, k), cap=cap, dropped=dropped)
        errors[seed] = dict(alive=int(res[-1]["alive"]), by_kind=res[-1]["by_kind"], dropped=int(dropped), capacity=cap,
                            spray_below=cfg["spray_below"], bubble_above=cfg["bubble_above"])
    finally:
        s.close()
    return None


@_reader_guard
def one_track_diffuse(seed, errors):
    """Two nrs_track_diffuse calls on record_for(pos) of tests/test_track_model_cpu.py at dt = 0.5 / track_model.stability, the fluid
    moved by upload between them (an upload through set_particles makes every slot new, so the record goes up again behind it), byte
    for byte against track_model.diffuse, walls included where the scene has them; channel 3 (kappa 0) unchanged bit for bit."""
    from tests import track_model as tm
    from tests.test_track_model_cpu import KAPPA, record_for
    sc = make_reader_scene(seed)
    tag = _reader_tag(sc, "track")
    s = _reader_context(sc)
    try:
        pos, vel = s.download()
        p = s.params
        walls = s.get("bSorted") if sc["bi"] is not None else None
        s.track_enable(capi.TRACK_ATTR)
        rec = record_for(np.where(np.isfinite(pos), pos, 0), s.real)
        bad_rows = np.flatnonzero(~np.isfinite(pos[:, :3]).all(axis=1))
        if len(bad_rows):   # "keeps its record" is its bytes: a + 0 would turn this -0.0 into +0.0
            rec[bad_rows[0], 0] = -0.0
        bits = np.uint64 if sc["double"] else np.uint32
        changed = 0
        for k in range(2):
            s.track_upload(capi.TRACK_ATTRIBUTE, rec)
            lam = tm.stability(p, pos, KAPPA, 1.0, sc["kset"], walls)
            dt = 0.5 / lam if lam > 0 and np.isfinite(lam) else float(p["timestep"][0])
            s.track_diffuse(KAPPA, dt)
            want = tm.diffuse(p, pos, rec, KAPPA, dt, sc["kset"], walls)
            got = s.track_result(capi.TRACK_ATTRIBUTE)
            if got.tobytes() != want.tobytes():
                bad = np.nonzero((got.view(bits) != want.view(bits)).any(axis=1))[0]
                return "%s call %d: %d of %d records differ, first %d: device %r model %r" % (tag, k, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])
            assert got[:, 3].tobytes() == rec[:, 3].tobytes(), tag + ": channel 3 (kappa 0) changed"
            assert got[bad_rows].tobytes() == rec[bad_rows].tobytes(), tag + ": the record of a non-finite particle changed"
            changed += int(np.count_nonzero(got[:, 0] != rec[:, 0]))
            rec = got
            if k == 0:
                pos = reader_moved(p, pos, vel, s.real)
                s.set_particles(pos, vel)
        assert changed > sc["n"] // 2, (tag, "the diffusion changed %d records in two calls" % changed)
        errors[seed] = dict(changed=changed, n=sc["n"])
    finally:
        s.close()
    return None


READERS = dict(sample=one_sample, surface=one_surface, aniso=one_aniso, diffuse=one_diffuse, track=one_track_diffuse)


if __name__ == "__main__":
    mode = sys.argv[3] if len(sys.argv) > 3 else ""
    if mode == "oracle":
        one = one_vs_oracle
    elif mode in EXACT_FLAG_SETS or mode in FAST_FLAG_SETS:
        one = (lambda sd, _f=dict(EXACT_FLAG_SETS, **FAST_FLAG_SETS)[mode]: one_flags(sd, _f))
    elif mode in SOLVERS:
        one = (lambda sd, _s=SOLVERS[mode]: one_pci(sd, _s))
    elif mode.endswith("-model") and mode[:-6] in SOLVERS:
        one = (lambda sd, _s=SOLVERS[mode[:-6]]: one_vs_model(sd, _s))
    elif mode in READERS:
        one = READERS[mode]
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    fails = div = 0
    for sd in range(first, first + seeds):
        r = one(sd)
        if r in ("diverged", "not comparable", "near cut"): div += 1
        elif r: print(r); fails += 1
        if (sd - first) % 25 == 24: print("... %d seeds done, %d failures" % (sd - first + 1, fails), flush=True)
    print("fuzz: %d seeds, %d failures, %d skipped (reference result not finite%s)" % (seeds, fails, div,
                                                                                    "; model: or a Monaghan pair near the cut" if mode.endswith("-model") else ""))
    sys.exit(1 if fails else 0)
