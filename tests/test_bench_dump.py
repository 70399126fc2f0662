"""bench.py --dump-outputs, host side: the arrays written, their dtypes, the size cap and the fixed row sample."""
import os

import numpy as np

import bench


def _state(n, real):
    rng = np.random.default_rng(7)
    return {"pos": rng.standard_normal((n, 4)).astype(real), "vel": rng.standard_normal((n, 4)).astype(real),
            "pressure": rng.standard_normal(n).astype(real)}


def test_small_state_is_written_whole(tmp_path):
    st = _state(1000, np.float32)
    bench.dump_outputs(str(tmp_path), st)
    assert sorted(os.listdir(tmp_path)) == ["pos.npy", "pressure.npy", "vel.npy"]
    for name, a in st.items():
        b = np.load(os.path.join(tmp_path, name + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(a, b)


def test_large_state_is_one_fixed_sample_under_the_cap(tmp_path):
    n, budget = 50000, 100000
    st = _state(n, np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), st, budget=budget)
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= budget + 3 * 256  # (.npy headers)
    rows = None
    for name, a in st.items():
        x, y = np.load(os.path.join(tmp_path, "a", name + ".npy")), np.load(os.path.join(tmp_path, "b", name + ".npy"))
        assert x.dtype == np.float64 and np.array_equal(x, y)
        assert len(x) == budget // (9 * 8) and x.shape[1:] == a.shape[1:]
        # the same rows of every array, in ascending order
        r = np.nonzero(np.isin(a[:, 0] if a.ndim == 2 else a, x[:, 0] if x.ndim == 2 else x))[0]
        assert np.array_equal(a[r], x)
        rows = r if rows is None else rows
        assert np.array_equal(r, rows)


def test_default_cap_is_under_64_mb():
    assert bench.DUMP_BYTES + 16 * 1024 <= 64 * 10 ** 6
