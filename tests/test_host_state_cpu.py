"""The array-state machine, the sort stage's choice, the step plan and the solver loops' exit rule (nereus_amd/csrc/nrs_host_state.h,
nrs_host_plan.h) without a GPU, through the program of tests/test_host_parts_cpu.py (tests/host_parts_main.cpp), plain and under
-fsanitize=address,undefined.

Every expectation restates the rule of the commit before the two headers existed, from its nrs_ctx_impl.h (Ctx::array_state, the six
transitions and the thirteen direct writes, Ctx::features / plan_step, Ctx::stage_prefix, Ctx::solve_loop, the `numCells > 8 n` test of
queue_resort_split and end_of_step); nothing is read from the code under test.

  * array_state: all 4096 combinations of the six bools it reads, slabOn, inplace and the four pointer facts, crossed with 129 count
    tuples: n one below, at, one above cap; nOwned and physN likewise against n; physN against cap; the known count against n and physN.
  * the transitions: every sequence of up to four of 23 (transition, arguments) pairs from the initial fields (292,561 sequences),
    field for field against a model, and the state each leaves under fixed facts.
  * plan_features / plan_step: the full cross product the module states at PLAN_AXES (8.8 M cases), against a vectorised model.
  * the sort choice: the prefix (compact first? prepared keys? re-sort? count known?) and the choice by mover count, with the counters.
  * solve_loop: iteration count, where measure was called, the last error, a failing measure.
"""
import subprocess

import numpy as np

from tests.test_host_parts_cpu import cmd, plain, refusal, run, sanitized  # noqa: F401  (plain, sanitized: fixtures)

E_HIP, E_STATE = -2, -4
RESORT_MIN, MAX_MOVER_PCT = 32768, 50  # the commit before: nrs_kernels_resort.h
FRESH, KEYS_READY, SPLIT_QUEUED, SLOT_ORDER, HOLES, INVALID = range(6)
STAGE_HASH, STAGE_SORT, STAGE_REORDER, STAGE_DENSITY, STAGE_FORCES = 1, 2, 3, 4, 5
SESPH, IISPH = 0, 1
(FLAG_REFERENCE_ORDER, FLAG_NO_FUSION, FLAG_NO_SHARED_LISTS, FLAG_FULL_SORT, FLAG_FAST_ARITH, FLAG_NO_WALL_WORKGROUPS,
 FLAG_STAGED_SCAN) = 1, 4, 8, 16, 32, 128, 256


# ---- array_state ---------------------------------------------------------------------------------------------------------------------
def state_model(b, n, cap, owned, phys, known):
    """Ctx::array_state of the commit before, on arrays of cases; b: the twelve bools in the order of the program's mask"""
    ready, pending, count_known, slot_order, classified, holes, slab, inplace, h_next, i_next, h_cur, movers = b
    out = np.full(ready.shape, -1, np.int64)

    def rule(cond, state):
        out[(out < 0) & cond] = state

    rule((n > cap) | (slab & (owned > n)), INVALID)
    rule(~slab & (holes | classified), INVALID)
    rule(ready & (~h_next | ~i_next), INVALID)
    rule(pending & (~ready | ~movers), INVALID)
    rule(count_known & ~pending, INVALID)
    rule(classified & (~slot_order | ~h_cur | ~h_next), INVALID)
    rule(slot_order & (~h_cur | ~h_next), INVALID)
    rule(holes & (~(inplace & ready & pending & count_known) | (phys < n) | (phys > cap) | (known > phys)), INVALID)
    rule(holes, HOLES)
    rule(count_known & (known > n), INVALID)
    rule(pending, SPLIT_QUEUED)
    rule(ready, KEYS_READY)
    rule(slot_order, SLOT_ORDER)
    rule(np.ones_like(ready), FRESH)
    return out


def count_tuples(cap=100):
    t = set()
    for n in (cap - 1, cap, cap + 1):
        for owned in (n - 1, n, n + 1):
            for phys in (n - 1, n, n + 1, cap - 1, cap, cap + 1):
                for known in (n - 1, n, n + 1, phys - 1, phys, phys + 1):
                    t.add((n, cap, owned, phys, known))
    return sorted(t)


def check_array_state(exe):
    tuples = count_tuples()
    assert len(tuples) == 129  # (of 3 * 3 * 6 * 6, many coincide)
    ans = run(exe, [cmd("astates", t) for t in tuples])
    m = np.arange(4096)
    b = [((m >> k) & 1).astype(bool) for k in range(12)]
    seen = set()
    for t, a in zip(tuples, ans):
        assert a[0] == "astates" and len(a[1]) == 4096, (t, a[0])
        got = np.frombuffer(a[1].encode(), np.uint8).astype(np.int64) - ord("0")
        want = state_model(b, *[np.int64(v) for v in t])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (t, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
        seen |= set(want.tolist())
    assert seen == {FRESH, KEYS_READY, SPLIT_QUEUED, SLOT_ORDER, HOLES, INVALID}


def test_array_state_truth_table(plain):
    check_array_state(plain)


# ---- transitions ---------------------------------------------------------------------------------------------------------------------
# the fields as a tuple: hashReady rsPending rsCountKnown slotOrderValid classifiedValid holesPending packedHashValid | rsKnownCount
# classifiedN physN
F0 = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
READY, PENDING, COUNT_KNOWN, SLOT, CLASSIFIED, HOLES_F, PACKED, KNOWN, CLASS_N, PHYS = range(10)


def put(f, **kw):
    f = f.copy()
    for k, v in kw.items():
        f[:, globals()[k]] = v
    return f


def transition(f, op, a, b):
    """the commit before: the six named transitions (0-5) and the writes at the eight sites that had none (6-14); f: one row of
    fields per case"""
    drop = lambda g: put(g, READY=0, PENDING=0, COUNT_KNOWN=0)
    fresh = lambda g: put(drop(g), SLOT=0, CLASSIFIED=0)
    known = lambda g, m: put(g, PENDING=1, COUNT_KNOWN=1, KNOWN=m)
    if op == 0:
        return drop(f)                                                   # drop_prepared_keys
    if op == 1:
        return fresh(f)                                                  # to_fresh
    if op == 2:
        return put(f, READY=1)                                           # keys_ready
    if op == 3:
        return put(f, PENDING=1)                                         # split_queued
    if op == 4:
        return known(f, a)                                               # split_queued_known
    if op == 5:
        return known(put(f, HOLES_F=1, PHYS=a, PACKED=1, READY=1), b)    # to_holes
    if op == 6:
        return put(f, HOLES_F=0)                                         # stage_prefix, before the reorder's gather
    if op == 7:
        return put(drop(put(f, HOLES_F=0)), PACKED=0)                    # compact_holes
    if op == 8:
        return put(fresh(f), PACKED=0)                                   # invalidate_grid_state (behind its compact_holes)
    if op == 9:
        return put(f, CLASSIFIED=0)                                      # sesph_tail, a fused launch
    if op == 10:
        return put(f, CLASSIFIED=1, CLASS_N=a)                           # sesph_tail, plan.classify
    if op == 11:
        return put(f, CLASSIFIED=0, SLOT=0)                              # slab_configure with other cuts
    if op == 12:
        return put(f, PACKED=a)                                          # finish_pack, compacting form
    if op == 13:                                                         # slab_unpack
        f = put(f, READY=f[:, PACKED])
        return put(f, PHYS=f[:, PHYS] + b, KNOWN=f[:, KNOWN] + b) if a else f
    if op == 14:
        return put(f, SLOT=a)                                            # end_of_step
    raise AssertionError(op)


OPS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (4, 7, 0), (5, 50, 7), (5, 40, 0), (6, 0, 0), (7, 0, 0), (8, 0, 0), (9, 0, 0),
       (10, 40, 0), (10, 50, 0), (11, 0, 0), (12, 0, 0), (12, 1, 0), (13, 0, 0), (13, 0, 5), (13, 1, 0), (13, 1, 5), (14, 0, 0), (14, 1, 0)]
DEPTH = 4
SEQ_N, SEQ_CAP, SEQ_OWNED = 45, 60, 45  # so that to_holes(50, 7) is AS_HOLES, (40, 0) has physN < n, three arrivals of 5 leave the capacity


def check_transitions(exe):
    assert sorted({o[0] for o in OPS}) == list(range(15))
    r = subprocess.run([exe], input=cmd("seqs", DEPTH, SEQ_N, SEQ_CAP, SEQ_OWNED, OPS) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert words[-2:] == ["seqs", "done"]
    got = np.array(words[:-2], np.int64).reshape(-1, 5)
    # the model, level by level in the program's order: a sequence is its prefix plus one transition
    level, levels = np.array([F0], np.int64), []
    for _ in range(DEPTH + 1):
        levels.append(level)
        level = np.stack([transition(level, *op) for op in OPS], axis=1).reshape(-1, len(F0))
    w = np.concatenate(levels)
    assert got.shape == (len(w), 5) and len(w) == sum(len(OPS) ** k for k in range(DEPTH + 1))
    bits = sum(w[:, k] << k for k in range(7))
    for name, g, x in (("bools", got[:, 0], bits), ("rsKnownCount", got[:, 1], w[:, KNOWN]), ("classifiedN", got[:, 2], w[:, CLASS_N]),
                       ("physN", got[:, 3], w[:, PHYS])):
        bad = np.nonzero(g != x)[0]
        assert bad.size == 0, (name, int(bad[0]), int(g[bad[0]]), int(x[bad[0]]))
    t = np.ones(len(w), bool)
    b = [w[:, k].astype(bool) for k in range(6)] + [t] * 6
    state = state_model(b, np.int64(SEQ_N), np.int64(SEQ_CAP), np.int64(SEQ_OWNED), w[:, PHYS], w[:, KNOWN])
    bad = np.nonzero(got[:, 4] != state)[0]
    assert bad.size == 0, ("state", int(bad[0]), int(got[bad[0], 4]), int(state[bad[0]]))
    assert set(state.tolist()) == {FRESH, KEYS_READY, SPLIT_QUEUED, SLOT_ORDER, HOLES, INVALID}


def test_transitions_against_model(plain):
    check_transitions(plain)


# ---- plan_features / plan_step -------------------------------------------------------------------------------------------------------
FLAGS = [FLAG_REFERENCE_ORDER, FLAG_NO_FUSION, FLAG_NO_SHARED_LISTS, FLAG_FULL_SORT, FLAG_FAST_ARITH, FLAG_NO_WALL_WORKGROUPS, FLAG_STAGED_SCAN]
STOPS = [0, STAGE_DENSITY, STAGE_FORCES]
CAPS = NS = [RESORT_MIN - 1, RESORT_MIN, RESORT_MIN + 1]
CELLS = [2 ** 30, 2 ** 30 + 1]
# the program's loops, outermost first: flag mask, solver, Muller kernels, fp32, mask of (qOk, pow2 grid, nearBitsValid, nb != 0, slabOn,
# ref), stop, cap, n, numCells
PLAN_AXES = (128, 5, 2, 2, 64, 3, 3, 3, 2)


def plan_model():
    fm, solver, muller, fp32, bm, i_stop, i_cap, i_n, i_cells = [np.ravel(x) for x in np.indices(PLAN_AXES, dtype=np.int32)]
    flag = lambda k: ((fm >> k) & 1).astype(bool)
    f_ref, f_nofuse, f_nolists, f_fullsort, f_fast, f_nowalls, f_staged = [flag(k) for k in range(7)]
    q_ok, pow2, near, walls, slab, ref_arg = [((bm >> k) & 1).astype(bool) for k in range(6)]
    muller, fp32 = muller.astype(bool), fp32.astype(bool)
    stop = np.array(STOPS)[i_stop]
    cap, n, cells = np.array(CAPS)[i_cap], np.array(NS)[i_n], np.array(CELLS, np.int64)[i_cells]
    sesph, iisph = solver == SESPH, solver == IISPH
    # Ctx::features
    ft_list_kernels = sesph | muller
    ft_lists = ft_list_kernels & ~(f_ref | f_nolists)
    ft_fast = ft_lists & f_fast & sesph & fp32 & muller
    ft_resort = ~(f_ref | f_nofuse | f_fullsort) & (cap >= RESORT_MIN)
    # Ctx::plan_step
    ref = ref_arg | f_ref | ~pow2
    quant = ft_lists & q_ok
    live = ~ref  # `if (s.ref) return s;`: everything below keeps its default, false
    lists = quant & (~sesph | (stop != STAGE_DENSITY))
    staged = f_staged & fp32 & muller & sesph & quant & (cells <= 2 ** 30)
    fast = ft_fast & lists
    wall_tiles = ~f_nowalls & near & walls & quant & ~staged
    wall_groups = wall_tiles & lists
    keys = (stop == 0) & ~f_nofuse & ~(iisph & slab)
    resort = keys & ft_resort & (n >= RESORT_MIN)
    watch = iisph & lists & ~slab
    cols = [ft_list_kernels, ft_lists, ft_fast, ft_resort, ref, quant, lists & live, wall_tiles & live, wall_groups & live, staged & live,
            fast & live, keys & live, resort & ~slab & live, resort & slab & live, watch & live]
    word = np.zeros(fm.shape, np.int64)
    for k, c in enumerate(cols):
        word |= c.astype(np.int64) << k
    return word


_plan_words = []


def check_plans(exe):
    if not _plan_words:
        _plan_words.append(plan_model())
    want = _plan_words[0]
    a = run(exe, [cmd("plans", FLAGS, STOPS, CAPS, NS, CELLS)])[0]
    assert a[0] == "plans" and len(a[1]) == 4 * want.size, (a[0], len(a[1]), want.size)
    d = np.frombuffer(a[1].encode(), np.uint8).astype(np.int64).reshape(-1, 4)
    d = np.where(d >= ord("a"), d - ord("a") + 10, d - ord("0"))
    got = (d[:, 0] << 12) | (d[:, 1] << 8) | (d[:, 2] << 4) | d[:, 3]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, np.unravel_index(int(bad[0]), PLAN_AXES), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    for k in range(15):  # every field is set in some case and clear in another
        col = (want >> k) & 1
        assert col.min() == 0 and col.max() == 1, k


def test_plan_cross_product(plain):
    check_plans(plain)


# ---- the sort choice -----------------------------------------------------------------------------------------------------------------
T_STALE = "coherent re-sort: mover count exceeds the particle count (stale count)"
MERGE_STAYERS, MERGE_MOVERS, FULL_SORT = range(3)


def few_movers(m, n):
    return m * 100 <= n * MAX_MOVER_PCT


def prefix_model(holes, ready, pending, known, m, stop, n):
    """Ctx::stage_prefix of the commit before, up to the sort: (compact first, prepared keys used, resort, count known), steps and
    fallbacks added"""
    steps = fallbacks = 0
    compact = False
    sorts = stop != STAGE_HASH and stop != STAGE_SORT
    if holes:
        can_merge = ready and pending and known and sorts and few_movers(m, n)
        if not can_merge:
            if ready and pending and known:
                steps, fallbacks = 1, 1
            compact = True
            ready = pending = known = False  # compact_holes drops the prepared keys
    return [int(compact), int(ready), int(ready and pending and sorts), int(known)], steps, fallbacks


def check_sort_choice(exe):
    cases, lines = [], []
    for n in (1000, 1001):
        for m in (0, 1, n // 2, n // 2 + 1, n, n + 1):
            lines.append(cmd("sortc", m, n))
            for mask in range(16):
                b = [(mask >> k) & 1 for k in range(4)]
                for stop in (0, STAGE_HASH, STAGE_SORT, STAGE_REORDER, STAGE_DENSITY):
                    cases.append(b + [m, stop, n])
    ans = run(exe, lines + [cmd("sortp", c) for c in cases])
    i = 0
    kinds = set()
    for n in (1000, 1001):
        for m in (0, 1, n // 2, n // 2 + 1, n, n + 1):
            rc, out = refusal(ans[i]), ans[i + 1]
            i += 2
            kind, steps, fallbacks, last = out[1].split()
            # the step is counted and the mover count recorded before the refusal
            assert out[0] == "sortc" and int(steps) == 1 and float.fromhex(last) == float(m), (m, n, out)
            if m > n:
                assert rc == (E_STATE, T_STALE) and int(fallbacks) == 0, (m, n, rc, out)
                continue
            want = (MERGE_STAYERS if m == 0 else MERGE_MOVERS) if few_movers(m, n) else FULL_SORT
            assert rc == (0, "") and int(kind) == want and int(fallbacks) == int(want == FULL_SORT), (m, n, rc, out)
            kinds.add(want)
    assert kinds == {MERGE_STAYERS, MERGE_MOVERS, FULL_SORT}
    assert few_movers(500, 1000) and not few_movers(501, 1000) and few_movers(500, 1001) and not few_movers(501, 1001)
    seen = set()
    for c, a in zip(cases, ans[i:]):
        want, steps, fallbacks = prefix_model(*c)
        v = a[1].split()
        assert a[0] == "sortp" and [int(t) for t in v[:4]] == want and (int(v[5]), int(v[6])) == (steps, fallbacks), (c, a)
        assert float.fromhex(v[7]) == -1.0                 # lastMovers is the sort's business
        if want[2] and want[3]:
            assert int(v[4]) == c[4], (c, a)               # the known count sizes the sort
        seen.add((tuple(want), steps))
    assert seen >= {((1, 0, 0, 0), 1), ((1, 0, 0, 0), 0), ((0, 1, 1, 1), 0), ((0, 1, 1, 0), 0), ((0, 1, 0, 0), 0), ((0, 0, 0, 0), 0)}


def test_sort_choice(plain):
    check_sort_choice(plain)


def check_sparse_cell_table(exe):
    cases = [(c, n) for n in (0, 1, 1000, 2 ** 27 - 1) for c in (8 * n - 1, 8 * n, 8 * n + 1) if c >= 0] + [(2 ** 31, 2 ** 27 - 1), (2 ** 31, 2 ** 28)]
    ans = run(exe, [cmd("sparse", c) for c in cases])
    for (c, n), a in zip(cases, ans):
        assert a == ("sparse", "%d" % int(c > 8 * n)), (c, n, a)


def test_sparse_cell_table(plain):
    check_sparse_cell_table(plain)


# ---- solve_loop ----------------------------------------------------------------------------------------------------------------------
ETA = 0.5


def loop_model(fixed, min_iters, cap, err_of, fail_at):
    """Ctx::solve_loop of the commit before: (rc, iterate calls, iters or None, last error or None, iterations after which measure ran)"""
    l, err, measured = 0, None, []
    while True:
        l += 1  # iterate(l - 1)
        last = l >= cap
        if fixed:
            if last:
                break
        elif l >= min_iters or last:
            measured.append(l)
            if l == fail_at:
                return E_HIP, l, None, err, measured
            err = err_of(l)
            if last or err <= ETA:
                break
    return 0, l, l, err, measured


def check_solve_loop(exe):
    cases = [(fixed, mn, cap, cross, fail) for fixed in (0, 1) for mn in range(5) for cap in range(1, 7) for cross in range(0, cap + 1)
             for fail in ([0] if fixed else range(0, cap + 1))]
    ans = run(exe, [cmd("loop", fixed, mn, cap, ETA, cross, fail) for fixed, mn, cap, cross, fail in cases])
    failed = 0
    for k, c in enumerate(cases):
        fixed, mn, cap, cross, fail = c
        rc, iterates, iters, err, measured = loop_model(fixed, mn, cap, lambda l: 0.25 if cross and l >= cross else 1.0 + l, fail)
        got_rc, v = refusal(ans[2 * k]), ans[2 * k + 1][1].split()
        assert got_rc == ((0, "") if rc == 0 else (E_HIP, "measure failed")), (c, got_rc)
        assert int(v[0]) == iterates and int(v[3]) == 1, (c, v)                       # iterate(0), iterate(1), ... and no more
        assert int(v[1]) == (12345 if iters is None else iters), (c, v)               # a failing measure returns at once
        assert float.fromhex(v[2]) == (-1.0 if err is None else err), (c, v)
        assert [int(t) for t in v[4:]] == measured, (c, v)
        if fixed:
            assert iterates == cap and not measured                                   # nothing read back
        else:
            assert all(l >= min(mn, cap) for l in measured)                           # none before min_iters
        failed += rc != 0
    assert failed > 0


def test_solve_loop(plain):
    check_solve_loop(plain)


def test_state_and_plan_under_sanitizers(sanitized):
    check_array_state(sanitized)
    check_transitions(sanitized)
    check_plans(sanitized)
    check_sort_choice(sanitized)
    check_sparse_cell_table(sanitized)
    check_solve_loop(sanitized)
