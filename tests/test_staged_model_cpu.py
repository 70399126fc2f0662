"""tests/staged_model.py on the targeted scenes of tests/test_staged_scan_gpu.py, without a GPU: every scene contains the branch of
k_density_staged (nrs_kernels_staged.h) it is named for, by the model's own figures — so that the GPU tests cannot pass vacuously —
and the model's pieces agree with independent brute-force forms."""
import numpy as np
import pytest

from tests import staged_model as sm


@pytest.fixture(scope="module")
def scenes():
    return sm.targeted_scenes()


@pytest.fixture(scope="module")
def models(scenes):
    return {k: sm.predict_scene(k, s) for k, s in scenes.items()}


def test_thresholds_are_the_smallest_floats_past_their_predicates():
    f = np.float32
    for ir in (0.0457, 0.0537, 0.1, 1.0, 0.013):
        ir = f(ir)
        t1, t2 = sm.make_thresholds(ir)
        below1, below2 = np.nextafter(t1, f(0)), np.nextafter(t2, f(0))
        assert np.sqrt(t1) >= ir and np.sqrt(below1) < ir
        h2 = f(ir * ir)
        assert f(np.sqrt(t2) * np.sqrt(t2)) > h2 and not f(np.sqrt(below2) * np.sqrt(below2)) > h2
        assert t1.dtype == f and t2.dtype == f and t1 <= t2


def test_hit_counts_equal_brute_force(scenes):
    """cells of at least h on grids of at least 4 cells: the 27-cell walk finds every pair within the cut-off exactly once, so the
    counts equal those of all pairs (same float arithmetic; scenes that lie inside the grid: all pairs do not wrap)"""
    for name in ("crowd_walls", "block_edge_walls", "hull_line", "wall_patch"):
        s = scenes[name]
        st = sm.oracle_state(name, s)
        n = len(s["pos"])
        nf, nb = sm.hit_counts(st["sortedPos"], st["hash"], st["cellStart"], st["cellEnd"], st["params"], n,
                               st.get("bCellStart"), st.get("bCellEnd"), st.get("sbi"))
        t_f, t_b = sm.make_thresholds(st["params"]["interactionRadius"][0])
        p = st["sortedPos"][:, :3]

        def brute(q, thr):
            d = p[:, None, :] - q[None, :, :]
            return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < thr

        np.testing.assert_array_equal(nf, brute(p, t_f).sum(axis=1) - 1, err_msg=name)
        np.testing.assert_array_equal(nb, brute(st["sbi"][:, :3], t_b).sum(axis=1) if "sbi" in st else 0, err_msg=name)


def test_wave_model_hulls_equal_per_lane_union(scenes):
    """the hull of a row, written differently: the smallest slot range that covers the x-1 .. x+1 cells of every lane of the wave"""
    for name in ("hull_sheet", "crowd", "tail129", "hull_pool_full"):
        s = scenes[name]
        st = sm.oracle_state(name, s)
        n = len(s["pos"])
        m = sm.wave_model(st["hash"], st["cellStart"], st["cellEnd"], None, st["params"], n)
        gs = [int(g) for g in st["params"]["gridSize"][0]]
        cells = {}
        for slot, h in enumerate(st["hash"][:n]):
            cells.setdefault(int(h), []).append(slot)
        for w in np.flatnonzero(~m["edge"]):
            for r in range(9):
                slots = []
                for h in st["hash"][w * 64:min(n, w * 64 + 64)]:
                    h = int(h)
                    cx, cy, cz = h % gs[0], (h // gs[0]) % gs[1], h // (gs[0] * gs[1])
                    for dx in (-1, 0, 1):
                        slots += cells.get(((cz + r // 3 - 1) * gs[1] + cy + r % 3 - 1) * gs[0] + cx + dx, [])
                assert m["hull"][w, r] == (max(slots) + 1 - min(slots) if slots else 0), (name, w, r)


def test_tail_scenes(models):
    for n in (1, 63, 64, 65, 129):
        for walls in ("", "_walls"):
            m = models["tail%d%s" % (n, walls)]
            assert len(m["staged"]) == (n + 63) // 64 and m["staged"].all() and m["stat_unstaged"] == 0
            assert m["lanes"][-1] == (n % 64 or 64)
            if walls and n > 1:
                assert m["nb"].max() > 0 and (m["wall_lanes"] > sm.COOP_LANES).any()
    assert models["tail65"]["lanes"][-1] == 1 and models["tail129"]["lanes"][-1] == 1 and models["tail63"]["lanes"][0] == 63


def test_edge_and_wrap_scenes(models, scenes):
    for walls in ("", "_walls"):
        n = len(scenes["block_interior" + walls]["pos"])
        a, b, c = (models[k + walls] for k in ("block_interior", "block_edge", "block_wrap"))
        assert a["stat_unstaged"] == 0 and not a["edge"].any()
        assert 0 < b["stat_unstaged"] < n and b["edge"].any() and b["staged"].any()
        assert 0 < c["stat_unstaged"] < n and c["edge"].any() and c["staged"].any()
        assert not b["over"].any() and b["stat_hit_max"] >= 8   # (lists that are read: the fall-back's results are checked through them)
    st = sm.oracle_state("block_wrap", scenes["block_wrap"])
    h = float(st["params"]["interactionRadius"][0])
    assert (scenes["block_wrap"]["pos"][:, 2] > 8 * h).any() and (scenes["block_wrap"]["pos"][:, 2] < 8 * h).any()   # half outside the grid


def test_hull_scenes(models):
    m = models["hull_line"]
    hull, st = m["hull"], m["staged"]
    assert st.all() and (hull[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()   # the eight other rows are empty
    assert ((hull[st, 4] > 64) & (hull[st, 4] <= 128)).any(), hull[:, 4]   # the second staging registers
    assert (hull[st, 4] > 128).any(), hull[:, 4]                           # the q = lane + 128 loop
    assert not m["over"].any() and m["stat_hit_max"] >= 8                  # every list is read
    m = models["hull_sheet"]
    assert m["staged"].any() and (~m["staged"] & ~m["edge"]).any()         # both sides of the pool test, no edge cell involved
    assert (m["plane"][~m["staged"]].max(axis=1) > sm.POOL).all() and not m["over"].any()
    m = models["hull_pool_full"]
    assert m["staged"].all() and (m["plane"][m["staged"]] == sm.POOL).any()   # exactly full: `<=`, not `<`
    assert (m["hull"] > 128).any() and ((m["hull"] > 64) & (m["hull"] <= 128)).any() and not m["over"].any()


def test_overflow_scenes(models):
    for name in ("crowd", "crowd_walls"):
        m = models[name]
        ps = m["particle_staged"]
        assert (m["over"] & ps).any() and (~m["over"] & ps).any() and m["staged"].any() and not m["staged"].all()
    m = models["crowd_walls"]
    ps = m["particle_staged"]
    # boundary hits alone exceed what is left above the fluid hits of a list that the fluid hits do not fill
    assert (ps & (m["nf"] <= sm.HIT_CAP) & (m["nb"] > sm.HIT_CAP - m["nf"])).any()
    assert (ps & ~m["over"] & (m["nb"] > 0)).any()


def test_wall_sweep_scenes(models):
    m = models["wall_patch"]
    wl, ps = m["particle_wall_lanes"], m["particle_staged"]
    coop = ps & (wl >= 1) & (wl <= sm.COOP_LANES)
    assert ((m["wall_lanes"] >= 1) & (m["wall_lanes"] <= sm.COOP_LANES) & m["staged"]).any()
    assert (coop & (m["nb"] > 0) & ~m["over"]).any()                                                  # a cooperative list that is read
    assert (coop & (m["nf"] < sm.HIT_CAP) & (m["nb"] > sm.HIT_CAP - m["nf"])).any()                   # ... and one with slot < nfL
    m = models["wall_floor"]
    assert ((m["wall_lanes"] > sm.COOP_LANES) & m["staged"]).any() and (m["particle_staged"] & ~m["over"] & (m["nb"] > 0)).any()


def test_2100_particle_boundary_cell_scenes(models, scenes):
    for name, coop in (("b2100_coop", True), ("b2100_lane", False)):
        s, m = scenes[name], models[name]
        st = sm.oracle_state(name, s)
        cnt = (st["bCellEnd"].astype(np.int64) - st["bCellStart"].astype(np.int64))[st["bCellStart"] != sm.EMPTY]
        assert list(cnt) == [2100]                      # ONE boundary cell, beyond the 11-bit offsets
        hit = m["nb"] > 0
        assert (hit & m["over"]).any() and m["particle_staged"][hit].all()
        wl = m["particle_wall_lanes"][hit]
        assert (wl <= sm.COOP_LANES).all() if coop else (wl > sm.COOP_LANES).all()
        # the packed count word (pack_counts, nrs_kernels_tiled.h): nb << 8 reaches the COUNTS_UNSTAGED diagnostic bit at 1024
        assert m["nb"].max() < 1024


def test_cut_off_pair_scenes(models, scenes):
    """the wall particle sits where the two cut-offs differ, and the statistics notice which one the launch applies"""
    f = np.float32
    for name, coop in (("cut_pair_coop", True), ("cut_pair_lane", False)):
        s, m = scenes[name], models[name]
        t_f, t_b = sm.make_thresholds(s["p"]["interactionRadius"][0])
        d = s["pos"][0, :3] - s["bi"][0, :3]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert d2.dtype == f and d2 == t_f and d2 < t_b and not d2 < t_f
        st = sm.oracle_state(name, s)
        own = int(np.flatnonzero(st["index"] == 0)[0])   # the owner's sorted slot
        assert m["nb"][own] == 1 and m["nb"].sum() == 1 and m["particle_staged"][own]
        tot = m["nf"] + m["nb"]
        assert m["stat_hit_max"] == tot[own] and (np.delete(tot, own) < tot[own]).all()   # one hit fewer changes STAT_HIT_MAX
        assert (m["particle_wall_lanes"][own] <= sm.COOP_LANES) == coop


def test_statistics_of_a_scene_by_hand():
    """three particles in one interior cell, two of them within h: no edge, one wave, lists of 1, 1 and 0"""
    p = sm.scene_params((4, 4, 4))
    h = float(p["interactionRadius"][0])
    s = dict(p=p, pos=sm._pts(np.array([[1.2, 1.2, 1.2], [1.5, 1.2, 1.2], [1.2, 1.95, 1.95]]) * h), bi=None, vbi=None)
    s["vel"] = np.zeros_like(s["pos"])
    m = sm.predict_scene("by_hand", s)
    assert m["stat_unstaged"] == 0 and m["stat_hit_overflow"] == 0 and m["stat_hit_max"] == 1
    assert sorted(m["nf"]) == [0, 1, 1] and m["hull"][0, 4] == 3 and m["hull"][0].sum() == 3
    s["pos"][2, :3] = np.array([3.5, 1.5, 1.5], np.float32) * h   # an edge cell on a grid of 4
    m = sm.predict_scene("by_hand_edge", s)
    assert m["stat_unstaged"] == 3 and m["edge"].all()
    s["pos"][2, 0] = np.nan                                        # cell 0: an edge cell; counted as an overflow
    m = sm.predict_scene("by_hand_nan", s)
    assert m["stat_unstaged"] == 3 and m["stat_hit_overflow"] == 1 and m["stat_hit_max"] == 1
