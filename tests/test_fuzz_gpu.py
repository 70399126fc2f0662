"""A slice of the randomised parity soak (tools/fuzz_parity.py): production kernels == reference-order kernels bit for bit on random
particle clouds with random grid geometry, wall sheets, precision, kernel set and solver."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_random_scenes_production_equals_reference_order(hip_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import one

    failures = []
    for seed in range(9000, 9150):   # (covers 11 narrow-x grids, 9 far origins, 8 scenes with NaN / inf coordinates)
        r = one(seed)                # ("diverged" is only returned under FUZZ_SKIP_NONFINITE=1: no seed is skipped here)
        if r:
            failures.append(r)
    assert not failures, failures[:3]


@pytest.mark.gpu
def test_random_slab_runs_equal_single_domain(hip_lib):
    """A slice of tools/fuzz_slab.py: 2-4 ranks as contexts of ONE process, random cuts / re-cuts / migrations.  Run as a child
    process: torch has to initialise its HIP runtime before libnereus_hip.so brings the system one into the process."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_slab.py"), "12", "7000"], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "12 seeds, 0 failures" in r.stdout and "'migrants': 0," not in r.stdout


@pytest.mark.gpu
def test_random_slab_runs_equal_single_domain_fp64(hip_lib):
    """tools/fuzz_slab.py in the fp64 builds, every second seed Monaghan: the end state equals the single domain's within
    TOL_STEPS_F64, after the oracle's run of each scene has shown no pair within 1e-11 m of the cut-off radius (a seed that fails this
    is replaced by the next one, not counted)."""
    import subprocess

    from tests.test_parity_gpu import TOL_STEPS_F64

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_slab.py"), "6", "7100", "sesph", "f64", "alternate", repr(TOL_STEPS_F64)],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "6 seeds, 0 failures, 0 skipped" in r.stdout and "'migrants': 0," not in r.stdout
    assert "largest difference f64 muller" in r.stdout and "largest difference f64 monaghan" in r.stdout


def _classes(seeds, solver):
    from fuzz_parity import make_scene
    c = dict(fp64=0, narrow_x=0, far=0, nonfinite=0, resort=0, walls=0, monaghan=0)
    for sd in seeds:
        sc = make_scene(sd, solver)
        c["fp64"] += sc["double"]
        c["narrow_x"] += sc["gs"][0] < 4
        c["far"] += sd % 17 == 16
        c["nonfinite"] += not np.all(np.isfinite(sc["pos"]))
        c["resort"] += sc["n"] >= 40000
        c["walls"] += sc["bi"] is not None
        c["monaghan"] += sc["kset"] == 0
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pcisph", "pbf"])
def test_random_scenes_pcisph_pbf_production_equals_reference_order(hip_lib, solver):
    """The soak's scenes with PCISPH / PBF (PBF: random eta, min_iters, relaxation, XSPH, tensile and vorticity settings): production
    kernels == reference-order kernels bit for bit at STAGE_P_ADVECT, at STAGE_P_SOLVE and after 3 steps (6 on the coherent re-sort
    seed).  Seeds 9000-9039 cover fp32 and fp64 (6 seeds), 3 narrow-x grids (1-2 cells: no quantised scan, no hit lists), 2 far origins
    (owners beyond the quanta's budget: wall workgroups' exact scan / far-owner path), 2 scenes with NaN / inf coordinates, 3 coherent
    re-sort seeds, wall sheets and both kernel sets."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import SOLVERS, one

    seeds = range(9000, 9040)
    c = _classes(seeds, SOLVERS[solver])
    assert c["fp64"] >= 5 and c["narrow_x"] >= 3 and c["far"] >= 2 and c["nonfinite"] >= 2 and c["resort"] >= 1 and c["walls"] >= 15, c
    failures = [r for r in (one(sd, SOLVERS[solver]) for sd in seeds) if r]
    assert not failures, failures[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pcisph", "pbf"])
def test_random_scenes_pcisph_pbf_device_equals_model(hip_lib, solver):
    """The device against the float64 models on pieces of the soak's scenes (tools/fuzz_parity.py one_vs_model): one fixed iteration,
    both paths, fp32 and fp64, Muller and Monaghan, far origins and wall sheets, PBF with random relaxation, XSPH and tensile settings;
    only geometry where the device's candidate rule is the models' (every cell edge >= h, every grid axis >= 4 cells, see
    make_model_scene).  A scene whose model result is not finite, or a Monaghan scene with a pair within 1e-5 of the cut-off h (where
    the truncated Monaghan W jumps, MONAGHAN_CUT_MARGIN), is not comparable: counted, at most 10 % of the slice."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import SOLVERS, make_model_scene, one_vs_model

    seeds = range(9100, 9140)
    scenes = [make_model_scene(sd, SOLVERS[solver]) for sd in seeds]
    assert sum(sc["double"] for sc in scenes) >= 5 and sum(sc["kset"] == 0 for sc in scenes) >= 10
    assert sum(sd % 17 == 16 for sd in seeds) >= 2 and sum(sc["bi"] is not None for sc in scenes) >= 15
    assert 5 <= sum(sc["ref"] for sc in scenes) <= 35
    assert all(min(sc["gs"]) >= 4 and np.all(sc["cs"] >= sc["h"]) for sc in scenes)
    results = [one_vs_model(sd, SOLVERS[solver]) for sd in seeds]
    failures = [r for r in results if r and r not in ("not comparable", "near cut")]
    assert not failures, failures[:3]
    skipped = results.count("not comparable") + results.count("near cut")
    assert skipped <= len(seeds) // 10, (results.count("not comparable"), results.count("near cut"))


ORACLE_CELLS = [dict(solver=sv, double=d, kset=k) for sv in (0, 1) for d in (False, True) for k in (1, 0)]   # (capi.SESPH / IISPH)


@pytest.mark.gpu
def test_random_scenes_against_oracle(hip_lib):
    """The soak's scenes against the CPU ORACLE (tools/fuzz_parity.py one_vs_oracle): one partial step, keys bit-exact, SESPH density /
    pressure / forces and every IISPH intermediate plus the iteration count, non-finite entries element for element, finite ones
    within the precision's bar.  Seeds 9200-9247 cycle through solver {SESPH, IISPH} x {fp32, fp64} x {Muller, Monaghan} (make_scene's
    config override; the rest of each scene is the seed's own): 6 scenes per cell, with walls, narrow-x grids, far origins, NaN / inf
    coordinates and coherent-re-sort sizes among them.  Only a seed whose oracle solve itself overflowed is not comparable: at most
    10 % of the slice."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import make_scene, one_vs_oracle

    seeds = list(range(9200, 9248))
    cfg = {sd: ORACLE_CELLS[i % len(ORACLE_CELLS)] for i, sd in enumerate(seeds)}
    scenes = {sd: make_scene(sd, config=cfg[sd]) for sd in seeds}
    for cell in ORACLE_CELLS:
        assert sum(all(sc[k] == v for k, v in cell.items()) for sc in scenes.values()) >= 3, cell
    assert sum(sc["bi"] is not None for sc in scenes.values()) >= 20
    assert sum(sc["gs"][0] < 4 for sc in scenes.values()) >= 3
    assert sum(sd % 17 == 16 for sd in seeds) >= 2
    assert sum(sc["n"] >= 40000 for sc in scenes.values()) >= 3
    del scenes
    errors, results = {}, {}
    for sd in seeds:
        results[sd] = one_vs_oracle(sd, config=cfg[sd], errors=errors)
    for k in sorted(errors):
        print("oracle slice max error solver=%d double=%d kset=%d %s: %.3g" % (k[0], k[1], k[2], k[3], errors[k]))
    failures = [r for r in results.values() if r and r != "not comparable"]
    assert not failures, failures[:3]
    skipped = [sd for sd, r in results.items() if r == "not comparable"]
    assert len(skipped) <= len(seeds) // 10, skipped


# ---- the launches selected by NRS_FLAG_STAGED_SCAN / NRS_FLAG_FAST_ARITH on the soak's scenes (tools/fuzz_parity.py one_flags) -------
FLAG_SEEDS = range(9300, 9348)
_flags_shared = {}   # per seed: the scene, the reference-order context's run and the oracle's, shared by the five flag sets


def _flag_classes():
    from fuzz_parity import FLAGS_CONFIG, make_scene
    c = dict(narrow_x=0, far=0, nonfinite=0, resort=0, walls=0, wrap=0, below_h=0, modes=[0, 0, 0])
    for sd in FLAG_SEEDS:
        sc = make_scene(sd, config=FLAGS_CONFIG)
        assert sc["solver"] == 0 and not sc["double"] and sc["kset"] == 1
        pos = sc["pos"][np.all(np.isfinite(sc["pos"]), axis=1), :3]
        lo = sc["p"]["worldOrigin"][0]
        hi = lo + np.array(sc["gs"]) * sc["p"]["cellSize"][0]
        c["narrow_x"] += sc["gs"][0] < 4
        c["far"] += sd % 17 == 16
        c["nonfinite"] += not np.all(np.isfinite(sc["pos"]))
        c["resort"] += sc["n"] >= 40000
        c["walls"] += sc["bi"] is not None
        c["wrap"] += bool(np.any((pos < lo) | (pos >= hi)))
        c["below_h"] += bool(np.any(sc["cs"] < sc["h"]))
        c["modes"][sc["dens_mode"]] += 1
    assert (c["narrow_x"] >= 3 and c["far"] >= 2 and c["nonfinite"] >= 2 and c["resort"] >= 3 and c["walls"] >= 25 and c["wrap"] >= 8
            and c["below_h"] >= 15), c
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("flag_set", ["staged", "staged+nofusion", "staged+fullsort"])
def test_random_scenes_staged_scan_equals_reference_order(hip_lib, flag_set):
    """The soak's scenes as fp32 Muller SESPH with NRS_FLAG_STAGED_SCAN (alone, unfused, with the full sort): density and pressure of
    the launches without shared lists (STAGE_DENSITY), density / pressure / forces at STAGE_FORCES, and the state after 3 steps (6 on
    the coherent-re-sort seeds) equal the reference-order context's bit for bit, NaN-aware.  Seeds 9300-9347: clumps, cells below h,
    grids the cloud wraps through, far origins, NaN / inf coordinates, wall sheets; on the narrow-x grids the plan ignores the flag,
    which must then change nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import EXACT_FLAG_SETS, one_flags

    _flag_classes()
    failures = [r for r in (one_flags(sd, EXACT_FLAG_SETS[flag_set], shared=_flags_shared) for sd in FLAG_SEEDS) if r]
    assert not failures, failures[:3]


def _record_fast_fuzz(flag_set, errors):
    from tests.test_fast_arith_gpu import record_drift   # (fast_arith_fuzz.json, next to its drift record)

    record_drift(flag_set, 1, None, None, file="fast_arith_fuzz.json", entry={"%d mode%d %s" % k: e for k, e in sorted(errors.items())})


@pytest.mark.gpu
@pytest.mark.parametrize("flag_set", ["fast", "fast+staged"])
def test_random_scenes_fast_arith_against_oracle(hip_lib, flag_set):
    """The same scenes with NRS_FLAG_FAST_ARITH (alone: k_forces_fast behind the default density launch; with NRS_FLAG_STAGED_SCAN: the
    FAST instantiations of the staged density launch too): hash, index and the cell tables equal the reference-order context's bit for
    bit; density and forces of one STAGE_FORCES against the CPU oracle (fp32, tait = double7), non-finite entries element for element,
    finite ones within 1e-5 array-relative: the density and the forces on every seed — the clump seeds (dens_mode 1, where large pair
    forces cancel) stayed within the bar when first measured (7.0e-7 at most), so fuzz_parity.FAST_FORCE_MODES names all three modes.
    The largest error of each quantity is printed per seed and per density mode and recorded next to the drift record of
    tests/test_fast_arith_gpu.py; DESIGN.md section 3 quotes the maxima."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import FAST_FLAG_SETS, FAST_FORCE_MODES, one_flags

    c = _flag_classes()
    assert c["modes"][1] >= 12 and sum(c["modes"][m] for m in FAST_FORCE_MODES) == len(FLAG_SEEDS), c   # every seed carries the force assertion
    errors, failures = {}, []
    for sd in FLAG_SEEDS:
        r = one_flags(sd, FAST_FLAG_SETS[flag_set], shared=_flags_shared, errors=errors)
        if r:
            failures.append(r)
    _record_fast_fuzz(flag_set, errors)
    for mode in (0, 1, 2):
        for nm in ("dens", "forces"):
            e = [v for (sd, m, q), v in errors.items() if m == mode and q == nm]
            print("%s dens_mode %d %s: max %.3g over %d seeds" % (flag_set, mode, nm, max(e) if e else 0.0, len(e)))
    assert not failures, failures[:3]
