"""The HIP-free parts of particle tracking (nereus_amd/csrc/nrs_host_track.h) without a GPU, through a stand-alone program
(tests/host_track_main.cpp) built with the host compiler, plain and under -fsanitize=address,undefined (a host program of its own:
nothing is preloaded): every refusal with its text; the id accounting — fresh ranges, next_id after an id upload, exhaustion at
0xfffffffe —, the saturating birth stamp, locate's range check, which slots an upload or a count change treats as new, the bytes of a
result — equal to the numpy model (tests/track_model.py).  And the ABI: the new symbols are declared, bound and exported.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import track_model as tm
from tests.test_host_inflow_cpu import line, no
from tests.test_host_parts_cpu import CXX, FLAGS, ROOT, SANITIZE, run

E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
ID, BIRTH, ATTRIBUTE, SLOT_OF = 0, 1, 2, 3


def _build(out, extra):
    subprocess.check_call([CXX] + FLAGS + ["-I", os.path.join(ROOT, "include")] + extra + ["-o", out, os.path.join(ROOT, "tests", "host_track_main.cpp")])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("host_track") / "host_track"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_track_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([CXX] + SANITIZE + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    return _build(str(d / "host_track"), SANITIZE)


OK = ("rc", "0")


def check_refusals(exe):
    assert run(exe, ["flags 0", "flags 1"]) == [OK] * 2
    for f in (2, 3, 0x80000000):
        no(run(exe, ["flags %d" % f])[0], E_INVALID, "unknown bits")
    no(run(exe, ["slabenable"])[0], E_INVALID, "slab context")
    no(run(exe, ["slabconfigure"])[0], E_INVALID, "nrs_slab_configure on a context that tracks")
    # refusal ON FLAGS MID IISPH NEEDATTR SETTLED
    assert run(exe, ["refusal 1 0 0 0 0 0", "refusal 1 1 1 1 1 0", "refusal 1 1 0 0 1 1", "refusal 1 0 1 1 0 0"]) == [OK] * 4
    for rest in ("0 0 0 0", "1 1 1 1", "0 0 1 1"):
        no(run(exe, ["refusal 0 1 " + rest])[0], E_STATE, "before nrs_track_enable")
    no(run(exe, ["refusal 1 0 0 0 1 0"])[0], E_STATE, "without NRS_TRACK_ATTR")
    no(run(exe, ["refusal 1 0 1 1 1 1"])[0], E_STATE, "without NRS_TRACK_ATTR")
    no(run(exe, ["refusal 1 1 1 0 0 1"])[0], E_STATE, "mid-update")
    no(run(exe, ["refusal 1 1 1 1 1 1"])[0], E_STATE, "mid-update")
    no(run(exe, ["refusal 1 1 0 1 0 1"])[0], E_STATE, "host-driven IISPH")
    # upload WHICH FLAGS HASSRC FIRST COUNT N
    assert run(exe, ["upload 0 0 1 0 10 10", "upload 1 0 1 3 7 10", "upload 2 1 1 9 1 10", "upload 0 0 0 10 0 10", "upload 0 0 1 0 0 0"]) == [OK] * 5
    no(run(exe, ["upload 3 1 1 0 1 10"])[0], E_INVALID, "NRS_TRACK_ID, NRS_TRACK_BIRTH or NRS_TRACK_ATTRIBUTE")
    no(run(exe, ["upload 9 1 1 0 1 10"])[0], E_INVALID, "NRS_TRACK_ID")
    no(run(exe, ["upload 2 0 1 0 1 10"])[0], E_STATE, "without NRS_TRACK_ATTR")
    for a in ("0 11 10", "4 7 10", "11 0 10", "10 1 10", "18446744073709551615 2 10", "1 18446744073709551615 10"):
        no(run(exe, ["upload 0 0 1 " + a])[0], E_INVALID, "inside [0, n)")
    no(run(exe, ["upload 0 0 0 0 1 10"])[0], E_INVALID, "src is NULL")
    # route WHICH FLAGS HAVELOCATE N LOCATED PRECISION
    assert run(exe, ["route 0 0 0 1080 0 32", "route 1 0 0 1080 0 64", "route 2 1 0 1080 0 32", "route 2 1 0 1080 0 64", "route 3 0 1 1080 257 32",
                     "route 3 0 1 5 0 32"]) == [("bytes", str(b)) for b in (4320, 4320, 17280, 34560, 1028, 0)]
    no(run(exe, ["route 4 1 1 10 10 32"])[0], E_INVALID, "which must be")
    no(run(exe, ["route 2 0 1 10 10 32"])[0], E_STATE, "without NRS_TRACK_ATTR")
    no(run(exe, ["route 3 1 0 10 10 32"])[0], E_STATE, "no nrs_track_locate")
    # the emit values, locate, diffuse
    assert run(exe, ["emitvalue -1 1", "emitvalue 0 1", "emitvalue 15 1"]) == [OK] * 3
    for s in (-2, 16, 2147483647, -2147483648):
        no(run(exe, ["emitvalue %d 1" % s])[0], E_INVALID, "slot")
    no(run(exe, ["emitvalue 0 0"])[0], E_INVALID, "NULL")
    assert run(exe, ["locate 0 0", "locate 0 %d" % tm.MAX_LOCATE, "locate 18446744073709551615 %d" % tm.MAX_LOCATE, "locate 4294967296 5"]) == [OK] * 4
    no(run(exe, ["locate 0 %d" % (tm.MAX_LOCATE + 1)])[0], E_INVALID, "2^27")
    no(run(exe, ["locate 0 18446744073709551615"])[0], E_INVALID, "2^27")
    good = [1.0, 0.0, 0.5, 2.0]
    assert run(exe, [line("diffuse", 1, good, 0.0), line("diffuse", 1, [0.0] * 4, 1e-3)]) == [OK] * 2
    no(run(exe, [line("diffuse", 0, good, 0.0)])[0], E_INVALID, "kappa is NULL")
    for c in range(4):
        for v in (-1.0, np.nan, np.inf, -np.inf):
            k = list(good)
            k[c] = v
            no(run(exe, [line("diffuse", 1, k, 0.0)])[0], E_INVALID, "kappa must be finite and >= 0")
    for v in (-1e-3, np.nan, np.inf):
        no(run(exe, [line("diffuse", 1, good, v)])[0], E_INVALID, "dt must be finite and >= 0")


def test_refusals(plain):
    check_refusals(plain)


def test_refusals_sanitized(sanitized):
    check_refusals(sanitized)


def check_accounting(exe):
    """a history of enables, appends, id uploads and count changes, answer by answer against the model"""
    # births saturate
    for steps in (0, 1, 7, 0xFFFFFFFE, 0xFFFFFFFF, 0x100000000, (1 << 64) - 1):
        assert run(exe, ["birth %d" % steps]) == [("b", str(tm.birth_of(steps)))]
    m = tm.State(1080, attr=False)
    lines, want = ["next 0", "reserve 1080"], [OK, ("ids", "0 1080")]

    def append(count):
        first = m.next_id
        m.append(count)
        lines.append("reserve %d" % count)
        want.append(("ids", "%d %d" % (first if count else first & 0xFFFFFFFF, m.next_id)))

    def upload(first, count):  # nrs_upload_particles: which slots are new
        n = m.n
        lines.append("freshupload %d %d %d" % (n, first, count))
        new = max(first + count - n, 0)
        want.append(("f", "%d %d" % (n, new)))
        append(new)
        assert m.n == max(n, first + count)

    def set_n(nn):
        n = m.n
        lines.append("freshsetn %d %d" % (n, nn))
        want.append(("f", "%d %d" % (min(n, nn), max(nn - n, 0))))
        if nn > n:
            append(nn - n)
        else:
            m.set_n(nn)

    append(42)
    append(0)
    upload(10, 100)        # inside: nothing new
    upload(m.n, 40)        # appended
    upload(m.n - 4, 8)     # straddles the old n
    upload(m.n + 5, 3)     # a gap: the gap's slots are new too
    set_n(500)
    set_n(500)
    set_n(700)
    ids = [7, 0xFFFFFFFD, 3000]
    m.upload_ids(ids, first=3)
    lines.append("uploaded 3 " + " ".join(str(i) for i in ids))
    want.append(("next", str(m.next_id)))
    m.upload_ids([5, 6], first=0)   # smaller ids leave next_id alone
    lines.append("uploaded 2 5 6")
    want.append(("next", str(m.next_id)))
    lines.append("uploaded 0")
    want.append(("next", str(m.next_id)))
    assert m.next_id == 0xFFFFFFFE and m.ids[500:].tolist() == list(range(1080 + 42 + 40 + 4 + 8, 1080 + 42 + 40 + 4 + 8 + 200))
    got = run(exe, lines)
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b]
    # exhaustion: the last id is 0xfffffffe; a refusal changes nothing
    tail = run(exe, ["next %d" % 0xFFFFFFFE, "uploaded 2 1 %d" % tm.NONE, "reserve 2", "reserve 0", "reserve 1", "reserve 0", "reserve 1",
                     "next %d" % 0xFFFFFFF0, "reserve 16", "reserve 15", "reserve 1", "next 0", "reserve 4294967296", "reserve 4294967295"])
    no(tail[1], E_INVALID, "NRS_TRACK_NONE is not an id")
    no(tail[2], E_CAPACITY, "particle ids exhausted; nrs_track_enable renumbers")
    assert tail[3] == ("ids", "%d %d" % (0xFFFFFFFE, 0xFFFFFFFE)) and tail[4] == ("ids", "%d %d" % (0xFFFFFFFE, 0xFFFFFFFF))
    assert tail[5][0] == "ids"
    no(tail[6], E_CAPACITY, "exhausted")
    no(tail[8], E_CAPACITY, "exhausted")
    assert tail[9] == ("ids", "%d %d" % (0xFFFFFFF0, 0xFFFFFFFF))
    no(tail[10], E_CAPACITY, "exhausted")
    no(tail[12], E_CAPACITY, "exhausted")
    assert tail[13] == ("ids", "0 4294967295")
    with pytest.raises(tm.Exhausted):
        tm.append(m.ids, m.birth, None, 0xFFFFFFFE, 2, 0, None)
    assert tm.append(m.ids[:0], m.birth[:0], None, 0xFFFFFFFE, 1, 0, None)[0].tolist() == [0xFFFFFFFE]


def test_accounting(plain):
    check_accounting(plain)


def test_accounting_sanitized(sanitized):
    check_accounting(sanitized)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
NEW = ["nrs_track_enable", "nrs_track_disable", "nrs_track_info", "nrs_track_upload", "nrs_track_result", "nrs_track_device_ptr",
       "nrs_track_emit_value", "nrs_track_locate", "nrs_track_diffuse"]


def test_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(NRS_[A-Z_]+) = (\d+)", code))
    assert enums["NRS_TRACK_ATTR"] == capi.TRACK_ATTR == 1
    assert (enums["NRS_TRACK_ID"], enums["NRS_TRACK_BIRTH"], enums["NRS_TRACK_ATTRIBUTE"], enums["NRS_TRACK_SLOT_OF"]) == (
        capi.TRACK_ID, capi.TRACK_BIRTH, capi.TRACK_ATTRIBUTE, capi.TRACK_SLOT_OF) == (0, 1, 2, 3)
    assert re.search(r"#define NRS_TRACK_NONE 0xffffffffu", code) and capi.TRACK_NONE == tm.NONE == 0xFFFFFFFF
    # the pinned enums did not grow
    assert sorted(v for k, v in enums.items() if k.startswith("NRS_STAT_")) == list(range(12))
    assert enums["NRS_STAGE_COUNT"] == 16
