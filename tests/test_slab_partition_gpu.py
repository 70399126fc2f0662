"""The slab partition on the device (nrs_kernels_slab.h: k_slab_count, k_slab_scan, k_slab_scatter in its three instantiations,
k_slab_headers, k_slab_append, k_slab_histogram, and the classification that rides in the fused force kernel) against the numpy
statement of the same operation (tests/slab_model.py), stream by stream and bit for bit: which slot went into which stream, in
which order, with which w tag, at which byte of the message, with which header — in fp32 and fp64, and for the sub-tile sweep in all
four builds (precision x kernel set: each is its own instantiation unit).

No torch: the message buffers are plain device allocations of the reference-name shim (allocateArray / copyArrayToDevice /
copyArrayFromDevice / freeArray), each with a tail of 4096 bytes behind nrs_slab_message_bytes(cap) and pre-filled with a byte
pattern, so that every byte the pack must not write — behind the filled prefix of either array, and behind the buffer — is checked.

Live particles (w == 1) with a non-finite x are left out of all inputs: the float-to-integer conversion of a NaN is not defined alike
on host and device (see tests/test_slab_model_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from nereus_amd import capi, slab
from nereus_amd.params import default_params
from tests import slab_model
from tests.slab_model import random_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL, PATTERN = 4096, 0xA5
E_INVALID, E_CAPACITY, E_STATE = "error -1:", "error -3:", "error -4:"
BUILDS = [(False, capi.MULLER), (False, capi.MONAGHAN), (True, capi.MULLER), (True, capi.MONAGHAN)]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]   # wavefront, sub-tile (256) and workgroup tile (2048) edges


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


_shim = None


def shim():
    global _shim
    if _shim is None:
        _shim = C.CDLL(os.path.join(ROOT, "nereus_amd", "libnereus_refshim.so"))
        _shim.allocateArray.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _shim.freeArray.argtypes = [C.c_void_p]
        _shim.copyArrayToDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _shim.copyArrayFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return _shim


class Buffer:
    """one message buffer on the device: `nbytes` of message + TAIL bytes, all PATTERN (or a given image)"""

    def __init__(self, nbytes, image=None):
        self.size = int(nbytes) + TAIL
        self.ptr = C.c_void_p()
        shim().allocateArray(C.byref(self.ptr), self.size)
        host = np.full(self.size, PATTERN, np.uint8)
        if image is not None:
            host[:len(image)] = image
        shim().copyArrayToDevice(self.ptr, host.ctypes.data_as(C.c_void_p), 0, self.size)

    def read(self):
        out = np.empty(self.size, np.uint8)
        shim().copyArrayFromDevice(out.ctypes.data_as(C.c_void_p), self.ptr, None, self.size)
        return out

    def free(self):
        if self.ptr:
            shim().freeArray(self.ptr)
            self.ptr = None


def solver(capacity, double=False, kset=capi.MULLER, iisph=False):
    return capi.Solver(default_params(1 if iisph else 0), max(1, int(capacity)), solver=capi.IISPH if iisph else capi.SESPH,
                       double=double, kernel_set=kset)


def real_of(double):
    return np.float64 if double else np.float32


def neighbours(p, lo, hi, halo, real, n_each, seed):
    """inputs of a left and a right neighbour slab (ids from 100000 / 200000)"""
    w = 2 * halo + 3
    pl, vl = random_input(seed + 1, n_each, lo - w, lo, halo, real, p)
    pr, vr = random_input(seed + 2, n_each, hi, hi + w, halo, real, p)
    vl[:, 3] += 100000
    vr[:, 3] += 200000
    return (pl, vl, lo - w, lo), (pr, vr, hi, hi + w)


def needed(p, lo, hi, halo, pos, real):
    s = slab_model.classify(p, lo, hi, halo, pos, real)
    return max(len(s["mig_l"]) + len(s["halo_l"]), len(s["mig_r"]) + len(s["halo_r"]), len(s["ghost"]))


def assert_image(buf, image, what):
    got = buf.read()
    assert got.shape == image.shape
    if not np.array_equal(got, image):
        bad = np.flatnonzero(got != image)
        raise AssertionError("%s: %d bytes differ from the model, first at byte %d of %d" % (what, len(bad), bad[0], len(got)))


def check_pack_unpack(s, pos, vel, lo, hi, halo, double, deferred, route=0, n_neigh=40, seed=0, pres=None, left=True, right=True,
                      slack=3, between=None):
    """upload-free core of most cases: `s` holds pos / vel (slot order) and is configured; pack, compare counts, messages and the
    untouched bytes with the model, unpack two model-made neighbour messages, compare download() and num_owned.  between(s, m), if
    given, is called between the pack and the unpack"""
    real = real_of(double)
    p = s.params
    (pl, vl, llo, lhi), (pr, vr, rlo, rhi) = neighbours(p, lo, hi, halo, real, n_neigh, seed)
    mvel = vel.copy()
    if pres is not None:
        mvel[:, 3] = pres   # IISPH: the warm-start pressure travels in vel.w
    cap = max(needed(p, lo, hi, halo, pos, real), needed(p, llo, lhi, halo, pl, real), needed(p, rlo, rhi, halo, pr, real), 1) + slack
    nl = slab_model.partition(p, llo, lhi, halo, pl, vl, real, cap=cap)
    nr = slab_model.partition(p, rlo, rhi, halo, pr, vr, real, cap=cap)
    m = slab_model.partition(p, lo, hi, halo, pos, mvel, real, cap=cap, left=left, right=right, pattern=PATTERN, tail=TAIL,
                             recv_left=nl.msg_right if left else None, recv_right=nr.msg_left if right else None)
    if not left and not right:
        m.pos, m.vel, m.n_owned = slab_model.unpack(m, None, None)
    assert not m.overflow
    nbytes = s.message_bytes(cap)
    assert nbytes == slab_model.message_bytes(cap, real)
    sl, sr = (Buffer(nbytes) if left else None), (Buffer(nbytes) if right else None)
    rl = Buffer(nbytes, nl.msg_right) if left else None
    rr = Buffer(nbytes, nr.msg_left) if right else None
    try:
        ptr = lambda b: None if b is None else b.ptr
        if deferred:
            assert s.slab_pack(ptr(sl), ptr(sr), cap, want_counts=False) is None
            counts = s.slab_last_counts()
        else:
            counts = s.slab_pack(ptr(sl), ptr(sr), cap)
            assert s.slab_last_counts() == counts
        assert counts == m.counts, (counts, m.counts)
        assert s.get_stat(capi.STAT_SLAB_PARTITION) == route
        assert s.n == m.counts[0] and s.n_owned == m.counts[0]
        s.synchronize()
        if left:
            assert_image(sl, m.msg_left, "left message")
        if right:
            assert_image(sr, m.msg_right, "right message")
        if between is not None:
            between(s, m)
        s.slab_unpack(ptr(rl), ptr(rr), cap)
        assert s.n == len(m.pos) and s.n_owned == m.n_owned
        if pres is None:
            gp, gv = s.download()
            want_v = m.vel
        else:
            gp, gv, gpres = s.download(pressure=True)
            want_v = m.vel.copy()
            want_v[:, 3] = 0
            assert np.array_equal(bits(gpres), bits(m.vel[:, 3]))          # every arrival's pressure is its message's vel.w
            assert np.array_equal(bits(s.get("pressure")[:len(m.pos)]), bits(m.vel[:, 3]))
        assert np.array_equal(bits(gp), bits(m.pos)), "positions after the unpack"
        assert np.array_equal(bits(gv), bits(want_v)), "velocities after the unpack"
        for rb, image in ((rl, nl.msg_right), (rr, nr.msg_left)):   # the received messages were only read
            if rb is not None:
                got = rb.read()
                assert np.array_equal(got[:len(image)], image) and np.all(got[len(image):] == PATTERN)
        return m
    finally:
        for b in (sl, sr, rl, rr):
            if b is not None:
                b.free()


def run_small_case(n, double, kset, lo, hi, halo, seed, iisph=False):
    real = real_of(double)
    for deferred in (False, True):
        s = solver(n + 8 * 64 + 64, double, kset, iisph)
        try:
            pos, vel = random_input(seed, n, lo, hi, halo, real, s.params)
            pres = None
            if iisph:
                pres = np.random.default_rng(seed).uniform(1.0, 5000.0, n).astype(real)
                vel[:, 3] = 0
            s.set_particles(pos, vel, pres)
            s.slab_configure(lo, hi, halo)
            if not deferred:
                with pytest.raises(capi.NereusError, match=E_STATE):
                    s.get_stat(capi.STAT_SLAB_PARTITION)   # no pack yet
            m = check_pack_unpack(s, pos, vel, lo, hi, halo, double, deferred, route=0, seed=seed, pres=pres)
            if not iisph and n:   # ids ride in vel.w
                ids = m.vel[:m.counts[0], 3].astype(np.int64)
                assert np.array_equal(ids, m.streams["stay"])
        finally:
            s.close()
    return m


@pytest.mark.parametrize("double,kset", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_compacting_scatter_sub_tile_edges_all_builds(hip_lib, n, double, kset):
    """k_slab_count / k_slab_scan / k_slab_scatter<R, false> / k_slab_headers / k_slab_append straight after an upload, at every edge
    of the wavefront, the 256-slot sub-tile and the 2048-slot workgroup tile; x random over [lo - halo - 2, hi + halo + 2) cells with
    a third of the entries dead (w in {2, 0, NaN}), every cut and halo face with nextafter in both directions, cells left of the world
    origin (lo - halo - 2 = -3)."""
    m = run_small_case(n, double, kset, lo=1, hi=7, halo=2, seed=1000 + n)
    if n >= 63:
        assert min(m.counts) > 0   # every stream is populated


@pytest.mark.parametrize("double", [False, True])
def test_scan_carry_600k_and_histogram(hip_lib, double):
    """N = 600,000 = 293 workgroups: k_slab_scan runs a second pass with a carry (more than 256 block counts per stream).  Pack only.
    nrs_slab_histogram on the same input against np.bincount: negative first_cell, bins that end inside the populated range, dead
    entries excluded."""
    real, n, lo, hi, halo = real_of(double), 600000, 1, 9, 2
    assert (n + 2047) // 2048 == 293
    s = solver(n, double)
    bufs = []
    try:
        p = s.params
        pos, vel = random_input(77, n, lo, hi, halo, real, p)
        s.set_particles(pos, vel)
        s.slab_configure(lo, hi, halo)
        first, nbins = -2, 9    # (populated: cells -3 .. 12)
        live = pos[:, 3] == 1
        cx = slab.cell_of(pos[live, 0], p["worldOrigin"][0][0], p["cellSize"][0][0], real=real) - first
        want = np.bincount(cx[(cx >= 0) & (cx < nbins)], minlength=nbins)
        assert cx.min() < 0 and cx.max() >= nbins and want.min() > 0
        assert np.array_equal(s.slab_histogram(first, nbins).astype(np.int64), want)
        cap = needed(p, lo, hi, halo, pos, real)
        m = slab_model.partition(p, lo, hi, halo, pos, vel, real, cap=cap, pattern=PATTERN, tail=TAIL)
        assert m.counts[5] < cap   # (the fuller message side sets cap: its last slot is written)
        nbytes = s.message_bytes(cap)
        bufs = [Buffer(nbytes), Buffer(nbytes)]
        assert s.slab_pack(bufs[0].ptr, bufs[1].ptr, cap, want_counts=False) is None
        assert s.slab_last_counts() == m.counts
        assert s.get_stat(capi.STAT_SLAB_PARTITION) == 0 and s.n == m.counts[0] == s.n_owned
        s.synchronize()
        assert_image(bufs[0], m.msg_left, "left message")
        assert_image(bufs[1], m.msg_right, "right message")
        gp, gv = s.download()
        assert np.array_equal(bits(gp), bits(m.stay_pos)) and np.array_equal(bits(gv), bits(m.stay_vel))
    finally:
        s.close()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("halo", [2, 8])
def test_minimum_width(hip_lib, double, halo):
    """hi - lo == 2 * halo: a particle is in stay, halo-left and halo-right at once; one cell narrower is refused"""
    lo, hi = 3, 3 + 2 * halo
    s = solver(64, double)
    try:
        with pytest.raises(capi.NereusError, match=E_INVALID):
            s.slab_configure(lo, hi - 1, halo)
    finally:
        s.close()
    m = run_small_case(257, double, capi.MULLER, lo, hi, halo, seed=2000 + halo)
    assert m.counts[0] > 0 and m.counts[0] == len(set(m.streams["halo_l"]) | set(m.streams["halo_r"]))
    if halo == 2:
        m = run_small_case(257, double, capi.MULLER, lo, hi + 1, halo, seed=2100)    # one column in neither halo
        assert m.counts[0] > len(set(m.streams["halo_l"]) | set(m.streams["halo_r"]))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_ends_of_the_chain(hip_lib, double, side):
    """send_left = NULL while particles do leave to the left (and the same on the right): the counts report them, n is the stay count,
    the other message, the ghosts and the arrivals are what they are with both neighbours"""
    real, n, lo, hi, halo = real_of(double), 2049, 1, 7, 2
    for deferred in (False, True):
        s = solver(n + 1024, double)
        try:
            pos, vel = random_input(31, n, lo, hi, halo, real, s.params)
            s.set_particles(pos, vel)
            s.slab_configure(lo, hi, halo)
            m = check_pack_unpack(s, pos, vel, lo, hi, halo, double, deferred, seed=31, left=side == "right", right=side == "left")
            assert m.counts[1] > 0 and m.counts[3] > 0 and m.counts[5] > 0
        finally:
            s.close()


@pytest.mark.parametrize("double", [False, True])
def test_message_capacity_to_the_last_slot_and_one_less(hip_lib, double):
    """cap == migrants + halo of the fuller side: no error, the last slot is written.  cap one less: the pack returns, the next call
    reports NRS_E_CAPACITY, the first cap entries are the model's, nothing behind either array or the buffer is written."""
    real, n, lo, hi, halo = real_of(double), 2049, 1, 7, 2
    s = solver(n + 1024, double)
    try:
        pos, vel = random_input(41, n, lo, hi, halo, real, s.params)
        p = s.params
        st = slab_model.classify(p, lo, hi, halo, pos, real)
        full = max(len(st["mig_l"]) + len(st["halo_l"]), len(st["mig_r"]) + len(st["halo_r"]))
        assert len(st["ghost"]) <= full - 1
        for cap in (full, full - 1):
            m = slab_model.partition(p, lo, hi, halo, pos, vel, real, cap=cap, pattern=PATTERN, tail=TAIL)
            nbytes = s.message_bytes(cap)
            bl, br = Buffer(nbytes), Buffer(nbytes)
            try:
                s.set_particles(pos, vel)
                s.slab_configure(lo, hi, halo)
                assert s.slab_pack(bl.ptr, br.ptr, cap, want_counts=False) is None    # the pack itself returns
                if cap == full:
                    assert not m.overflow and s.slab_last_counts() == m.counts
                else:
                    assert m.overflow
                    with pytest.raises(capi.NereusError, match=E_CAPACITY):
                        s.slab_unpack(None, None, cap)
                    assert s.slab_last_counts() == m.counts
                s.synchronize()
                assert_image(bl, m.msg_left, "left message, cap %d of %d" % (cap, full))
                assert_image(br, m.msg_right, "right message, cap %d of %d" % (cap, full))
            finally:
                bl.free()
                br.free()
    finally:
        s.close()


@pytest.mark.parametrize("double", [False, True])
def test_guarded_error_paths(hip_lib, double):
    """Ghost overflow alone (no neighbour buffers, more than cap migrants within the halo): NRS_E_CAPACITY.  A received header with
    nm + nh > cap: NRS_E_INVALID.  Arrivals beyond the context capacity: NRS_E_CAPACITY.  Guarded paths: nothing here writes out of
    bounds."""
    real, n, lo, hi, halo = real_of(double), 2049, 1, 7, 2
    s = solver(n, double)
    try:
        p = s.params
        pos, vel = random_input(51, n, lo, hi, halo, real, p)
        # ghost overflow ALONE: stayers only in the interior (no halo copies), 100 migrants within the halo on either side, so that
        # each message side (100) fits cap = 150 and only the ghost array (200) does not
        ox, cs = real(p["worldOrigin"][0][0]), real(p["cellSize"][0][0])
        rng = np.random.default_rng(52)
        cells = np.concatenate([rng.uniform(lo + halo + 0.1, hi - halo - 0.1, 300), rng.uniform(lo - halo + 0.1, lo - 0.1, 100),
                                rng.uniform(hi + 0.1, hi + halo - 0.1, 100)])
        gpos = np.ones((500, 4), real)
        gpos[:, 0] = (ox + cs * rng.permutation(cells)).astype(real)
        gvel = np.zeros((500, 4), real)
        gvel[:, 3] = np.arange(500)
        st = slab_model.classify(p, lo, hi, halo, gpos, real)
        want = [len(st[k]) for k in slab_model.STREAMS]
        assert want == [300, 100, 0, 100, 0, 200]
        for cap, fits in ((200, True), (150, False)):
            s.set_particles(gpos, gvel)
            s.slab_configure(lo, hi, halo)
            if fits:
                assert s.slab_pack(None, None, cap) == want
            else:
                with pytest.raises(capi.NereusError, match=E_CAPACITY):
                    s.slab_pack(None, None, cap)
                assert s.slab_last_counts() == want
        # corrupt header
        cap = n
        s.set_particles(pos, vel)
        s.slab_pack(None, None, cap)
        image = slab_model.message_image(pos[:0], vel[:0], pos[:0], vel[:0], cap, real)
        image[:16].view(np.uint32)[:] = (cap, 1, 0, 0)
        rb = Buffer(len(image), image)
        try:
            with pytest.raises(capi.NereusError, match=E_INVALID):
                s.slab_unpack(rb.ptr, None, cap)
        finally:
            rb.free()
        # arrivals beyond the context capacity: stay + ghosts + n migrants > n
        s.set_particles(pos, vel)
        s.slab_pack(None, None, cap)
        live = pos[pos[:, 3] == 1]
        image = slab_model.message_image(live[:0], live[:0], pos[:0], vel[:0], cap, real)
        image[:16].view(np.uint32)[:] = (cap, 0, 0, 0)
        rb = Buffer(len(image), image)
        try:
            with pytest.raises(capi.NereusError, match=E_CAPACITY):
                s.slab_unpack(None, rb.ptr, cap)
        finally:
            rb.free()
    finally:
        s.close()


@pytest.mark.parametrize("double", [False, True])
def test_iisph_pressure_rides_in_vel_w(hip_lib, double):
    """IISPH, N = 2049, halo 8: on pack vel.w of both messages is the uploaded warm-start pressure of that particle; after the unpack
    the pressure of every arrival is its message's vel.w (k_pressure_to_velw / k_velw_to_pressure in either precision)"""
    run_small_case(2049, double, capi.MULLER, lo=1, hi=19, halo=8, seed=61, iisph=True)


# ---- in-place and pre-classified scatter ---------------------------------------------------------------------------------------
def block_scene(real, seed=5):
    """a jittered 34^3 block (39,304 particles) with x velocities that carry particles across the cuts in one step; ids in vel.w"""
    from nereus_amd import scene

    p = default_params(0)
    pos = scene.fluid_block(34, 34, 34, float(p["interactionRadius"][0]), real=real, jitter=0.25)
    n = len(pos)
    assert n == 39304
    rng = np.random.default_rng(seed)
    vel = np.zeros_like(pos)
    vel[:, 0] = np.where(rng.random(n) < 0.5, 3.0, -3.0)
    vel[:, 1:3] = rng.normal(0, 0.2, (n, 2))
    vel[:, 3] = np.arange(n)
    return pos.astype(real), vel.astype(real)


def block_cuts(p, pos, real):
    """Two cuts through the block that keep this rank above RESORT_MIN_PARTICLES (32,768): the outermost cell column on the left and
    the four outermost on the right belong to the neighbours.  (A single cut through the middle would leave 19,652 particles, below
    the size from which the partition works in place: the routes under test would not be taken.)  With the block's jitter, particles
    sit within one step's travel of both faces."""
    cx = slab.cell_of(pos[:, 0], p["worldOrigin"][0][0], p["cellSize"][0][0], real=real)
    lo, hi = int(cx.min()) + 1, int(cx.max()) - 3
    assert ((cx >= lo) & (cx < hi)).sum() >= 33000
    return lo, hi


def to_stepped_state(double, route):
    """route 2: configure, pack / unpack with no neighbour data, one step (whose force kernel classifies for the next partition).
    route 0: the same, then the right cut moves by one cell, which discards the classification (nrs_slab_configure: "partition the
    slow way once").  route 1: one single-domain step first, then configure: slot order and keys of the fused step without a
    classification, the in-place scatter classifies itself."""
    real = real_of(double)
    pos, vel = block_scene(real)
    s = solver(len(pos) + 4096, double)
    p = s.params
    lo, hi = block_cuts(p, pos, real)
    s.set_particles(pos, vel)
    if route == 1:
        s.step(1)
        s.slab_configure(lo, hi, 2)
    else:
        s.slab_configure(lo, hi, 2)
        c = s.slab_pack(None, None, 16384)
        assert c[1] > 0 and c[3] > 0 and 0 < c[5] < c[1] + c[3]
        s.slab_unpack(None, None, 16384)
        assert s.n == c[0] + c[5] >= 32768 and s.n_owned == c[0]
        s.step(1)
        if route == 0:
            hi -= 1
            s.slab_configure(lo, hi, 2)
    spos, svel = s.download()
    assert np.isfinite(spos).all() and len(spos) >= 32768
    return s, spos, svel, lo, hi


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("route", [2, 1, 0])
def test_in_place_and_pre_classified_scatter(hip_lib, double, route):
    """k_slab_scatter<R, true, true> (route 2: streams from the force kernel's classification), k_slab_scatter<R, true> (route 1) and
    the compacting fallback after a re-cut (route 0) on a stepped 34^3 block: NRS_STAT_SLAB_PARTITION proves the route, the model's
    input is the download() taken after the step.  Messages, ghosts, counts and arrivals bit for bit; the stay stream in slot order
    (compact_holes is stable, nrs_ctx_impl.h)."""
    s, spos, svel, lo, hi = to_stepped_state(double, route)
    try:
        m = check_pack_unpack(s, spos, svel, lo, hi, 2, double, deferred=False, route=route, n_neigh=300, seed=70 + route)
        assert m.counts[1] > 0 and m.counts[3] > 0 and m.counts[5] > 0 and m.counts[2] > 0 and m.counts[4] > 0
        if route != 1:
            assert (spos[:, 3] == 2).sum() > 0   # last exchange's ghosts are among the slots and are dropped
    finally:
        s.close()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("route", [2, 1])
def test_step_after_in_place_partition_merges(hip_lib, double, route):
    """after an in-place partition (deferred counts, no neighbour data) the next step consumes the holes through the coherent
    re-sort: resort_stats shows one more merged step, and the state is finite"""
    s, spos, svel, lo, hi = to_stepped_state(double, route)
    try:
        real, p = real_of(double), s.params
        m = slab_model.partition(p, lo, hi, 2, spos, svel, real, cap=16384, left=False, right=False)
        before = s.resort_stats()
        assert s.slab_pack(None, None, 16384, want_counts=False) is None
        s.slab_unpack(None, None, 16384)
        assert s.slab_last_counts() == m.counts and s.get_stat(capi.STAT_SLAB_PARTITION) == route
        assert s.n == m.counts[0] + m.counts[5] and s.n_owned == m.counts[0]
        s.step(1)
        after = s.resort_stats()
        assert after[0] - after[1] == before[0] - before[1] + 1, (before, after)
        gp, gv = s.download()
        assert len(gp) == m.counts[0] + m.counts[5] and np.isfinite(gp).all() and np.isfinite(gv).all()
        own = gp[:, 3] == 1
        want = np.sort(np.concatenate([svel[m.streams["stay"], 3]]))
        assert own.sum() == m.counts[0] and np.array_equal(np.sort(gv[own, 3]), want)   # ids of the owned particles
    finally:
        s.close()


# ---- call sequences around an exchange -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("first", ["compacting", "in_place"])
def test_pack_right_after_a_pack_nobody_finished(hip_lib, double, first):
    """nrs_slab_pack(counts = NULL) and at once the next pack: the second call reads the first one's totals itself (and, after an
    in-place first pack, compacts its holes) and partitions what the first one kept — the model's stay stream, in slot order.  The
    second pack takes the compacting form; its counts, messages, ghosts and arrivals are the model's bit for bit."""
    real = real_of(double)
    if first == "in_place":
        s, pos, vel, lo, hi = to_stepped_state(double, 2)
        halo, cap, n_neigh = 2, 16384, 300
    else:
        lo, hi, halo, cap, n_neigh = 1, 7, 2, 2049, 40
        s = solver(2049 + 1024, double)
        pos, vel = random_input(91, 2049, lo, hi, halo, real, s.params)
        s.set_particles(pos, vel)
        s.slab_configure(lo, hi, halo)
    try:
        m1 = slab_model.partition(s.params, lo, hi, halo, pos, vel, real, cap=cap, left=False, right=False)
        assert not m1.overflow and 0 < m1.counts[0] < len(pos) and m1.counts[1] > 0 and m1.counts[3] > 0
        assert s.slab_pack(None, None, cap, want_counts=False) is None
        m2 = check_pack_unpack(s, m1.stay_pos, m1.stay_vel, lo, hi, halo, double, deferred=False, route=0, n_neigh=n_neigh, seed=92)
        assert m2.counts[0] == m1.counts[0] and m2.counts[1] == m2.counts[3] == m2.counts[5] == 0 and m2.counts[2] > 0 and m2.counts[4] > 0
    finally:
        s.close()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("route", [2, 1])
def test_download_between_in_place_pack_and_unpack(hip_lib, double, route):
    """an in-place pack, then download() — which compacts the holes: the stay stream in slot order — and only then the unpack: the
    arrivals go behind the compacted particles, and the arrays are the model's bit for bit as in the plain sequence"""
    s, spos, svel, lo, hi = to_stepped_state(double, route)

    def download_the_stayers(s, m):
        gp, gv = s.download()
        assert np.array_equal(bits(gp), bits(m.stay_pos)) and np.array_equal(bits(gv), bits(m.stay_vel))
        assert s.n == m.counts[0] == s.n_owned

    try:
        m = check_pack_unpack(s, spos, svel, lo, hi, 2, double, deferred=False, route=route, n_neigh=300, seed=80 + route,
                              between=download_the_stayers)
        assert m.counts[1] > 0 and m.counts[3] > 0 and m.counts[5] > 0 and len(m.pos) > m.n_owned > m.counts[0]
    finally:
        s.close()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("route", [2, 1])
def test_new_grid_origin_after_in_place_exchange(hip_lib, double, route):
    """an in-place pack and unpack (the arrays keep their holes), then nrs_set_params with another grid origin: the prepared keys and
    the queued split are void, the holes are compacted at once — download() gives the model's arrays after the unpack — and the next
    step hashes and sorts from scratch (no step of the coherent re-sort is counted) and keeps every particle"""
    s, spos, svel, lo, hi = to_stepped_state(double, route)
    try:
        real, p = real_of(double), s.params
        m = slab_model.partition(p, lo, hi, 2, spos, svel, real, cap=16384, left=False, right=False)
        want_pos, want_vel, n_owned = slab_model.unpack(m, None, None)
        assert s.slab_pack(None, None, 16384, want_counts=False) is None
        s.slab_unpack(None, None, 16384)
        assert s.get_stat(capi.STAT_SLAB_PARTITION) == route and s.n == len(want_pos) and s.n_owned == n_owned == m.counts[0]
        q = s.params
        q["worldOrigin"][0][0] -= real(0.25) * q["cellSize"][0][0]   # a quarter cell: every particle stays inside the grid
        cx = slab.cell_of(want_pos[:, 0], q["worldOrigin"][0][0], q["cellSize"][0][0], real=real)
        assert cx.min() >= 1 and cx.max() < int(q["gridSize"][0][0]) - 1
        s.set_params(q)
        assert s.n == len(want_pos) and s.n_owned == n_owned
        gp, gv = s.download()
        assert np.array_equal(bits(gp), bits(want_pos)) and np.array_equal(bits(gv), bits(want_vel))
        before = s.resort_stats()
        s.step(1)
        assert s.resort_stats() == before
        gp, gv = s.download()
        assert len(gp) == len(want_pos) and np.isfinite(gp).all() and np.isfinite(gv).all()
        assert np.array_equal(np.sort(gv[:, 3]), np.sort(want_vel[:, 3]))   # ids: nobody lost, nobody twice
    finally:
        s.close()
