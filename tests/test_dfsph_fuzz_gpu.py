"""DFSPH on slices of the randomised parity soak (tools/fuzz_parity.py): production kernels == reference-order kernels bit for bit on
the soak's random scenes, and the device against tests/dfsph_model.py on pieces of them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_random_scenes_dfsph_production_equals_reference_order(hip_lib):
    """Seeds 9000-9039 with DFSPH (random eta and minimum of both loops, the divergence solve on or off, warm start on or off): at
    STAGE_P_ADVECT, at STAGE_P_SOLVE and after 3 steps (6 on the coherent re-sort seeds), fp32 and fp64, narrow-x grids, far origins,
    NaN / inf coordinates, wall sheets and both kernel sets."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import SOLVERS, make_scene, one

    seeds = range(9000, 9040)
    scenes = [make_scene(sd, SOLVERS["dfsph"]) for sd in seeds]
    assert sum(sc["double"] for sc in scenes) >= 5 and sum(sc["n"] >= 40000 for sc in scenes) >= 1
    assert sum(sc["cfg"]["min_v"] == 0 for sc in scenes) >= 3 and sum(sc["cfg"]["warm"] == 0 for sc in scenes) >= 3
    assert sum(sc["cfg"]["eta"] == 0 for sc in scenes) >= 3 and sum(sc["cfg"]["eta"] > 0 for sc in scenes) >= 3
    failures = [r for r in (one(sd, SOLVERS["dfsph"]) for sd in seeds) if r]
    assert not failures, failures[:3]


@pytest.mark.gpu
def test_random_scenes_dfsph_device_equals_model(hip_lib):
    """Seeds 9100-9139: one fixed iteration per loop, both paths, fp32 and fp64, Muller and Monaghan, wall sheets, the scene's
    velocities, against the model with the bars of tests/test_dfsph_gpu.py.  Every position of a DFSPH step is a start position, which
    the model takes from the device, so its cut-off decisions are the device's (no Monaghan near-cut skips)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_parity import SOLVERS, make_model_scene, one_vs_model

    seeds = range(9100, 9140)
    scenes = [make_model_scene(sd, SOLVERS["dfsph"]) for sd in seeds]
    assert sum(sc["double"] for sc in scenes) >= 5 and sum(sc["kset"] == 0 for sc in scenes) >= 10
    assert sum(sc["bi"] is not None for sc in scenes) >= 15 and 5 <= sum(sc["ref"] for sc in scenes) <= 35
    results = [one_vs_model(sd, SOLVERS["dfsph"]) for sd in seeds]
    failures = [r for r in results if r and r != "not comparable"]
    assert not failures, failures[:3]
    assert results.count("not comparable") <= len(seeds) // 10
