"""The HIP-free parts of the sources and sinks (nereus_amd/csrc/nrs_host_inflow.h) without a GPU, through a stand-alone program
(tests/host_inflow_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): every refusal with its text; the frame, the spacing, the sites (through the row tables the kernel searches), the
schedule with its counts, the origins and positions of sites, and the predicate with its bounds — byte-equal to the numpy model
(tests/inflow_model.py).  And the ABI: the new symbols are declared, bound and exported, the pinned enums unchanged.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import inflow_model as im
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, floats, hx, refusal, run
from tests.test_inflow_model_cpu import DT, DT_TWO, FAUCET, S, params, sink_scene

E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
MASS, RHO = 0.04772199, 1000.0


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + ["-I", os.path.join(ROOT, "include")] + extra + ["-o", out, os.path.join(ROOT, "tests", "host_inflow_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_inflow") / "host_inflow"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_inflow_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_inflow"), SANITIZE)


def line(name, *vals):
    """a command line: Python ints travel as decimals, everything else as hex floats"""
    out = [name]
    for v in vals:
        for x in (v if isinstance(v, (list, tuple, np.ndarray)) else [v]):
            out.append(str(int(x)) if isinstance(x, (int, np.integer, bool)) else hx(float(x)))
    return " ".join(out)


def no(ans, code, part):
    c, msg = refusal(ans)
    assert c == code and part in msg and len(msg) > 0, (ans, code, part)


def emitter_line(shape=im.RECT, enabled=1, center=(0.0, 0.0, 0.0), direction=(0.0, -1.0, 0.0), half_extent=(0.1, 0.1), speed=1.0, spacing=0.05,
                 max_particles=0, mass=MASS, rho=RHO):
    he = list(np.broadcast_to(np.asarray(half_extent, np.float64), (2,)))
    return line("emitter", int(shape), int(enabled), [float(x) for x in center], [float(x) for x in direction], [float(x) for x in he], float(speed),
                float(spacing), int(max_particles), float(mass), float(rho))


# ---- every refusal, with its text ---------------------------------------------------------------------------------------------------------
def check_refusals(exe):
    assert run(exe, ["slot 0", "slot 15"]) == [("rc", "0")] * 2
    no(run(exe, ["slot 16"])[0], E_INVALID, "slot")
    no(run(exe, ["slot 4294967295"])[0], E_INVALID, "slot")
    bad = [(dict(shape=2), "shape"), (dict(center=(np.nan, 0, 0)), "finite"), (dict(direction=(0, np.inf, 0)), "finite"),
           (dict(half_extent=(np.nan, 0.1)), "finite"), (dict(half_extent=(0.1, np.inf)), "finite"), (dict(speed=np.nan), "finite"),
           (dict(spacing=np.inf), "finite"), (dict(direction=(0.0, 0.0, 0.0)), "direction has no length"), (dict(speed=-1.0), "speed"),
           (dict(spacing=-0.1), "spacing must be >= 0"), (dict(half_extent=(-0.1, 0.1)), "half_extent"), (dict(half_extent=(0.1, -0.1)), "half_extent"),
           (dict(spacing=1e-6, half_extent=(1.0, 1.0)), "2^24"), (dict(spacing=1e-3, half_extent=(2.1, 2.1)), "2^24"),
           (dict(spacing=1e-3, half_extent=(2.4, 0.0), shape=im.DISC), "2^24"), (dict(spacing=0.0, mass=0.0), "particleMass"),
           (dict(spacing=0.0, rho=0.0), "particleMass")]
    for kw, part in bad:
        no(run(exe, [emitter_line(**kw)])[0], E_INVALID, part)
    # the largest layers that are accepted: 4095 x 4095 sites of a rectangle; a disc's second extent is not looked at
    assert run(exe, [emitter_line(spacing=1e-3, half_extent=(2.0475, 2.0475))])[0][0] == "e"
    assert run(exe, [emitter_line(shape=im.DISC, half_extent=(0.1, -5.0))])[0][0] == "e"
    assert run(exe, [emitter_line(speed=0.0, enabled=0)])[0][0] == "e"
    # sinks
    box = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    assert run(exe, [line("sinks", 1, 1, 0, 0, 1, box), line("sinks", 0, 0, 7, 0, 0), line("sinks", 1, 16, 1, 0, 16, box * 16)]) == [("rc", "0")] * 3
    no(run(exe, [line("sinks", 2, 0, 1, 0, 0)])[0], E_INVALID, "flags")
    no(run(exe, [line("sinks", 0, 17, 1, 0, 16, box * 16)])[0], E_INVALID, "nboxes")
    no(run(exe, [line("sinks", 0, 0, 1, 1, 0)])[0], E_INVALID, "reserved")
    for a in range(3):
        b = list(box)
        b[a] = b[3 + a]
        no(run(exe, [line("sinks", 0, 1, 1, 0, 1, b)])[0], E_INVALID, "min < max")
        b[a] = 2.0
        no(run(exe, [line("sinks", 0, 2, 1, 0, 2, box + b)])[0], E_INVALID, "min < max")
        b = list(box)
        b[a] = np.nan
        no(run(exe, [line("sinks", 0, 1, 1, 0, 1, b)])[0], E_INVALID, "finite")
        b = list(box)
        b[3 + a] = np.inf
        no(run(exe, [line("sinks", 0, 1, 1, 0, 1, b)])[0], E_INVALID, "finite")
    # the state
    assert run(exe, ["refusal 0 0 0 0", "refusal 0 0 0 1", "refusal 0 0 1 0"]) == [("rc", "0")] * 3
    no(run(exe, ["refusal 1 0 0 0"])[0], E_INVALID, "slab context")
    no(run(exe, ["refusal 1 1 1 1"])[0], E_INVALID, "slab context")
    no(run(exe, ["refusal 0 1 0 0"])[0], E_STATE, "mid-update")
    no(run(exe, ["refusal 0 0 1 1"])[0], E_STATE, "host-driven IISPH")
    no(run(exe, ["slabrefuse"])[0], E_INVALID, "nrs_slab_configure on a context with sources or sinks")
    # the block
    good = dict(o=[0.0, 0.0, 0.0], sp=[0.1, 0.1, 0.1], dims=[7, 5, 3], v=[0.0, 0.0, 0.0])

    def blk(hasl=1, hasv=1, n=0, cap=1000, **kw):
        g = dict(good)
        g.update(kw)
        return line("block", int(hasl), g["o"], g["sp"], g["dims"], int(hasv), g["v"], int(n), int(cap))
    assert run(exe, [blk(), blk(n=895), blk(cap=105)]) == [("nodes", "105")] * 3
    no(run(exe, [blk(n=896)])[0], E_CAPACITY, "capacity - n")
    no(run(exe, [blk(cap=104)])[0], E_CAPACITY, "capacity - n")
    no(run(exe, [blk(hasl=0)])[0], E_INVALID, "lattice is NULL")
    no(run(exe, [blk(hasv=0)])[0], E_INVALID, "vel is NULL")
    no(run(exe, [blk(v=[0.0, np.nan, 0.0])])[0], E_INVALID, "vel is not finite")
    no(run(exe, [blk(dims=[7, 0, 3])])[0], E_INVALID, "dim of 0")
    no(run(exe, [blk(sp=[0.1, -0.1, 0.1])])[0], E_INVALID, "spacing")
    no(run(exe, [blk(o=[np.inf, 0.0, 0.0])])[0], E_INVALID, "origin")


def test_refusals(plain):
    check_refusals(plain)


def test_refusals_sanitized(sanitized):
    check_refusals(sanitized)


# ---- frame, sites, schedule, positions: byte-equal to the model ------------------------------------------------------------------------------
EMITTERS = [
    dict(FAUCET),
    dict(center=(0.1, 0.2, 0.3), direction=(0.3, -0.2, 0.9), half_extent=(3.2 * S, 1.7 * S), speed=2.5, spacing=0.0, shape=im.RECT),
    dict(center=(-0.5, 0.25, 1.0), direction=(1.0, 1.0, 1.0), half_extent=0.2, speed=0.7, spacing=0.013, shape=im.DISC),
    dict(center=(0.0, 0.0, 0.0), direction=(-5.0, 0.1, 0.1), half_extent=(0.0, 0.31), speed=3.0, spacing=0.1, shape=im.RECT),
    dict(center=(0.0, 1.0, 0.0), direction=(0.0, 0.0, 1.0), half_extent=7.0 * S, speed=1.0, spacing=S, shape=im.DISC),  # (7, 0) lies on the rim
]


def check_emitter_against_model(exe, kw):
    p = params()
    m = im.Emitter(p, **kw)
    setl = emitter_line(mass=float(p["particleMass"][0]), rho=float(p["restDensity"][0]), **kw)
    q = 0.25 * m.s / m.speed  # (the faucet's DT, DT_TWO; the same fractions of a spacing for the others: 7 layers or more, room for 5)
    dts = [q, q, 2.3 * m.s / m.speed, q, 3.7 * m.s / m.speed, q, q]
    assert kw != FAUCET or (q == DT and dts[2] == DT_TWO)
    room = 5 * len(m.ij) + 3
    lines = [setl, "sites"]
    for dt in dts:
        lines.append(line("step", float(dt), int(room)))
        room -= len(m.ij) * len(m.schedule(dt, room))
    ans = run(exe, lines)
    word, rest = ans[0]
    assert word == "e", ans[0]
    t = rest.split()
    assert float.fromhex(t[0]) == m.s and int(t[1]) == len(m.ij)
    got = np.array([float.fromhex(x) for x in t[2:]])
    assert got.tobytes() == np.concatenate([m.d, m.e1, m.e2]).tobytes()
    assert ans[1][0] == "ij" and np.array(ans[1][1].split(), np.int64).reshape(-1, 2).tolist() == m.ij.tolist()
    # the schedule again, answer by answer
    m2 = im.Emitter(p, **kw)
    room = 5 * len(m.ij) + 3
    offsets = []
    for dt, (word, rest) in zip(dts, ans[2:]):
        offs = m2.schedule(dt, room)
        room -= len(m.ij) * len(offs)
        t = rest.split()
        assert word == "l" and [int(x) for x in t[:4]] == [len(offs), room, m2.emitted, m2.dropped], (t, offs, room)
        assert [float.fromhex(x) for x in t[4:]] == [m2.acc] + offs
        offsets += offs
    assert m2.dropped > 0 and m2.emitted > 0  # (the room runs out: both branches are taken)
    # origins and positions of a few sites of every emitted layer, both precisions
    lines, want = [], []
    pick = sorted(set([0, len(m.ij) // 3, len(m.ij) // 2, len(m.ij) - 1]))
    for off in offsets[:4]:
        lines.append(line("origin", float(off)))
        want.append(m.center + off * m.d)
        for prec, real in ((32, np.float32), (64, np.float64)):
            pos, _ = m.layer(off, real)
            for k in pick:
                lines.append(line("pos", prec, float(off), int(m.ij[k, 0]), int(m.ij[k, 1])))
                want.append(pos[k, :3].astype(np.float64))
    for (word, rest), w in zip(run(exe, [setl] + lines)[1:], want):
        assert floats(rest).tobytes() == np.asarray(w, np.float64).tobytes(), (word, rest, w)


@pytest.mark.parametrize("which", range(len(EMITTERS)))
def test_emitter_matches_model(plain, which):
    check_emitter_against_model(plain, EMITTERS[which])


def test_emitter_matches_model_sanitized(sanitized):
    for kw in EMITTERS:
        check_emitter_against_model(sanitized, kw)


# ---- the predicate ------------------------------------------------------------------------------------------------------------------------------
def check_predicate(exe):
    for double in (False, True):
        real, prec = (np.float64, 64) if double else (np.float32, 32)
        p, sc, pos, vel, box = sink_scene(double)
        lo, hi = im.domain(p, real)
        rng = np.random.default_rng(5)
        pts = np.concatenate([pos[::37], pos[-1:], rng.uniform(-2.0, 2.0, (40, 4)).astype(real),
                              np.array([[np.nan, 0, 0, 1], [0, -np.inf, 0, 1], [0, 0, np.inf, 1], [lo[0], lo[1], lo[2], 1], [hi[0], 0, 0, 1],
                                        [0, np.nextafter(hi[1], real(0)), 0, 1], [box[0], box[1], box[2], 1], [box[3], box[4], box[5], 1],
                                        [0.1, real(box[1]), 0.1, 1], [0.1, np.nextafter(real(box[1]), real(0)), 0.1, 1]], real)])
        geo = [[float(p["worldOrigin"][0][a]) for a in range(3)], [int(p["gridSize"][0][a]) for a in range(3)], [float(p["cellSize"][0][a]) for a in range(3)]]
        for flags, boxes in ((1, [box]), (0, [box]), (1, []), (0, []), (1, [box, [-2.0, -2.0, -2.0, 0.0, 0.0, 0.0]])):
            set_line = line("sinks", flags, len(boxes), 1, 0, len(boxes), [x for b in boxes for x in b])
            ans = run(exe, [set_line] + [line("caught", prec, *geo, [float(x) for x in r[:3]]) for r in pts])
            assert ans[0] == ("rc", "0")
            want = im.caught(p, pts, real, boxes=boxes, domain_on=bool(flags))
            got = np.array([int(rest.split()[0]) for _, rest in ans[1:]], bool)
            assert got.tolist() == want.tolist()
            assert 0 < want.sum() < len(pts)
            assert floats(ans[1][1].split(" ", 1)[1]).tobytes() == np.concatenate([lo, hi]).astype(np.float64).tobytes()
        # no sinks at all: only the non-finite rows
        ans = run(exe, ["nosinks"] + [line("caught", prec, *geo, [float(x) for x in r[:3]]) for r in pts])
        assert [int(rest.split()[0]) for _, rest in ans[1:]] == (~np.isfinite(pts[:, :3]).all(axis=1)).astype(int).tolist()
    assert run(exe, ["due 1 0", "due 1 1", "due 2 3", "due 3 3", "due 6 3", "due 7 3"]) == [("due", x) for x in "110110"]


def test_predicate(plain):
    check_predicate(plain)


def test_predicate_sanitized(sanitized):
    check_predicate(sanitized)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
NEW = ["nrs_emitter_set", "nrs_emitter_get", "nrs_emit_block", "nrs_sinks_set", "nrs_cull", "nrs_sinks_count"]


def test_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.NrsEmitter) == 96 and C.sizeof(capi.NrsSinkConfig) == 16 + 16 * 6 * 8
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_[A-Z_]+) = (\d+)", code))
    assert enums["NRS_MAX_EMITTERS"] == capi.MAX_EMITTERS == 16 and enums["NRS_MAX_SINK_BOXES"] == capi.MAX_SINK_BOXES == 16
    assert (enums["NRS_EMITTER_RECT"], enums["NRS_EMITTER_DISC"], enums["NRS_SINK_DOMAIN"]) == (capi.EMITTER_RECT, capi.EMITTER_DISC, capi.SINK_DOMAIN) == (0, 1, 1)
    # the pinned enums did not grow
    assert sorted(v for k, v in enums.items() if k.startswith("NRS_STAT_")) == list(range(12))
    assert enums["NRS_STAGE_COUNT"] == 16
