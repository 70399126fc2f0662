"""Akinci surface tension and adhesion without a GPU: the model's two kernels against the reference's own outputs (committed fixture),
the antisymmetry of the fluid terms on a random blob, and the new symbol in the header and the built library."""
import os
import re

import numpy as np

from nereus_amd import capi
from tests import akinci_model as M
from tests import ref_pin
from tests.oracle_lib import IISPH, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_kernels_pin.npz")


def test_model_kernels_equal_reference_fixture():
    """d1_*_f6 / _f7 are the outputs of the reference's Cakinci / Aboundary in its fp64 build.  Cakinci: fp64 roundoff (the model forms
    the same products; a few ulp of the largest term cover any reassociation).  Aboundary: 2 * 2^-23 relative, the reference rounds
    through powf; NaN sites (a radicand roundoff left below zero) are excluded by mask and must be NaN in the model too; out of branch
    both are exactly 0."""
    g = np.load(GOLD)
    for hi, h in enumerate(g["radii"]):
        tag = "d1_h%d" % hi
        r = np.ascontiguousarray(g[tag + "_r"])
        k1, k2 = ref_pin.constants(6, float(h), 1)
        bp = ref_pin.constants(7, float(h), 1)[0]
        want = g[tag + "_f6"][:, 0]
        got = M.cakinci(r, float(h), k1, k2)
        ln = M._len(r).astype(np.float64)
        out = ~((ln > 0) & (ln <= h))
        assert np.all(got[out] == 0) and np.all(want[out] == 0)
        scale = abs(k1) * max(abs(k2), float(h) ** 6 / 64)   # the largest term of either branch
        assert np.max(np.abs(got - want)) <= 8 * np.finfo(np.float64).eps * scale
        assert np.count_nonzero(want) > 100
        want = g[tag + "_f7"][:, 0]
        got = M.aboundary(r, float(h), bp)
        out = ~((2.0 * ln > h) & (ln <= h))
        assert np.all(got[out] == 0) and np.all(want[out] == 0)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        ok = ~nan & ~out
        assert np.count_nonzero(ok) > 100
        assert np.all(np.abs(got[ok] - want[ok]) <= 2 * 2.0 ** -23 * np.abs(want[ok]))
        # the force walk's form: 0 at the NaN sites, within the same bound elsewhere
        cl = M.aboundary(r, float(h), bp, clamp=True)
        assert np.all(cl[nan] == 0) and np.all(np.abs(cl[ok] - want[ok]) <= 2 * 2.0 ** -23 * np.abs(want[ok]))


def test_model_kernels_in_fp32_equal_reference_fixture():
    """The model evaluates both kernels with the device's operations in the build's precision; in float32 that is the reference's fp32
    build (d0_*): Cakinci bit for bit, Aboundary NaN exactly where the fixture has NaN (it holds such sites) and within 2 * 2^-23."""
    g = np.load(GOLD)
    nans = 0
    for hi, h in enumerate(g["radii"]):
        tag = "d0_h%d" % hi
        r = np.ascontiguousarray(g[tag + "_r"])
        k1, k2 = ref_pin.constants(6, float(h), 0)
        bp = ref_pin.constants(7, float(h), 0)[0]
        want = g[tag + "_f6"][:, 0]
        got = M.cakinci(r, float(h), k1, k2, np.float32).astype(np.float32)
        np.testing.assert_array_equal(ref_pin.bits(got), ref_pin.bits(np.ascontiguousarray(want)))
        want = g[tag + "_f7"][:, 0].astype(np.float64)
        got = M.aboundary(r, float(h), bp, np.float32)
        nan = np.isnan(want)
        nans += int(nan.sum())
        assert np.array_equal(np.isnan(got), nan)
        assert np.all(np.abs(got[~nan] - want[~nan]) <= 2 * 2.0 ** -23 * np.abs(want[~nan]))
        assert np.all(M.aboundary(r, float(h), bp, np.float32, clamp=True)[nan] == 0)
    assert nans > 0


def random_blob(n=400, seed=11, double=True):
    p = Oracle.default_params(IISPH, double)
    h = float(p["interactionRadius"][0])
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.2 * h, 2.2 * h, (n, 3)) + np.array([0.3, 0.2, -0.1])
    return p, x


def test_fluid_terms_are_antisymmetric():
    """No boundaries: the pair terms of F^coh + F^curv are exactly antisymmetric, so their sum over the blob is N eps of roundoff:
    |sum F| <= 1e-10 sum |F_i|."""
    p, x = random_blob()
    rho = M.density(p, x)
    m = M.run(p, x, rho, 1.0, 0.0)
    f = m["coh"] + m["curv"]
    per = np.linalg.norm(f, axis=1)
    assert len(m["ii"]) > 10 * len(x) and per.max() > 0
    assert np.linalg.norm(m["coh"], axis=1).max() > 0 and np.linalg.norm(m["curv"], axis=1).max() > 0
    assert np.linalg.norm(f.sum(axis=0)) <= 1e-10 * per.sum()
    assert np.all(m["adh"] == 0)


def test_cohesion_pulls_a_pair_together_and_adhesion_pulls_at_the_wall():
    """signs of the definition: two particles at 0.8 h attract each other; a particle at 0.75 h above one boundary particle is pulled
    towards it, at 1.2 h it feels nothing"""
    p = Oracle.default_params(IISPH, True)
    h = float(p["interactionRadius"][0])
    x = np.array([[0.0, 0.0, 0.0], [0.8 * h, 0.0, 0.0]])
    m = M.run(p, x, np.full(2, 1000.0), 1.0, 0.0)
    assert m["coh"][0, 0] > 0 and m["coh"][1, 0] < 0
    b = np.array([[0.0, 0.0, 0.0]])
    for d, pulled in ((0.75, True), (1.2, False)):
        m = M.run(p, np.array([[0.0, d * h, 0.0]]), np.full(1, 1000.0), 0.0, 1.0, b, np.array([1e-5]))
        assert (m["adh"][0, 1] < 0) == pulled and (pulled or np.all(m["adh"] == 0))


def test_symbol_and_header():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+nrs_set_surface_akinci\s*\(\s*nrs_ctx\s*\*\s*ctx\s*,\s*double\s+gamma\s*,\s*double\s+beta_adhesion\s*\)\s*;", code)
    assert re.search(r"\bNRS_ARR_NORMALS\s*=\s*34\b", code)
    lib = capi.load_library()
    assert hasattr(lib, "nrs_set_surface_akinci")
    assert capi.ARRAYS["normals"] == (34, "v4")
