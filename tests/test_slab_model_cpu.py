"""tests/slab_model.py, the numpy statement of the slab partition that the gloo protocol tests and the device tests share, against the
partition code the checker engine carried before it was rewritten on the model, and against the properties every partition has.

Live particles (w == 1) with a non-finite x are left out of every input here and in tests/test_slab_partition_gpu.py: the
float-to-integer conversion of a NaN is not defined alike on host and device, so such a particle has no stream the two could agree on
(non-finite coordinates on slab contexts are not supported)."""
import numpy as np
import pytest

from nereus_amd import slab
from nereus_amd.params import default_params, params_dtype
from tests import slab_model
from tests.slab_model import random_input


def legacy_pack(p, lo, hi, halo, cap, pos, vel):
    """OracleSlabEngine.pack as it was before it used the model (float32): counts, the two (header, pos, vel), ghosts, stayers"""
    ox, cs = float(p["worldOrigin"][0][0]), float(p["cellSize"][0][0])
    live = pos[:, 3] == 1.0
    pos, vel = pos[live], vel[live]
    cx = slab.cell_of(pos[:, 0], ox, cs)
    stay = (cx >= lo) & (cx < hi)
    mig_l, mig_r = cx < lo, cx >= hi
    halo_l = stay & (cx < lo + halo)
    halo_r = stay & (cx >= hi - halo)
    ghost = (mig_l & (cx >= lo - halo)) | (mig_r & (cx < hi + halo))

    def tag(a):
        a = a.copy()
        a[:, 3] = 2.0
        return a

    msgs = []
    for mig, hal in ((mig_l, halo_l), (mig_r, halo_r)):
        nm, nh = int(mig.sum()), int(hal.sum())
        assert nm + nh <= cap
        bp, bv = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32)
        bp[:nm], bv[:nm] = pos[mig], vel[mig]
        bp[nm:nm + nh], bv[nm:nm + nh] = tag(pos[hal]), vel[hal]
        msgs.append((np.array([nm, nh, 0, 0], np.uint32), bp, bv))
    counts = [int(stay.sum()), int(mig_l.sum()), int(halo_l.sum()), int(mig_r.sum()), int(halo_r.sum()), int(ghost.sum())]
    return counts, msgs, (tag(pos[ghost]), vel[ghost]), (pos[stay], vel[stay])


def legacy_unpack(stay, ghost, msgs):
    mig_p, mig_v, hal_p, hal_v = [], [], [], []
    for m in msgs:
        if m is None:
            continue
        hdr, bp, bv = m
        nm, nh = int(hdr[0]), int(hdr[1])
        mig_p.append(bp[:nm].copy()); mig_v.append(bv[:nm].copy())
        hal_p.append(bp[nm:nm + nh].copy()); hal_v.append(bv[nm:nm + nh].copy())
    owned_p = np.concatenate([stay[0]] + mig_p)
    owned_v = np.concatenate([stay[1]] + mig_v)
    return np.concatenate([owned_p, ghost[0]] + hal_p), np.concatenate([owned_v, ghost[1]] + hal_v), len(owned_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_engines_former_partition(seed):
    p = default_params(0)
    rng = np.random.default_rng(100 + seed)
    halo = int(rng.choice([2, 8]))
    lo = int(rng.integers(-6, 10))
    hi = lo + 2 * halo + int(rng.integers(0, 9))
    n = int(rng.choice([0, 1, 65, 700, 5000]))
    pos, vel = random_input(seed, n, lo, hi, halo, np.float32, p)
    cap = n + 1
    counts, msgs, ghost, stay = legacy_pack(p, lo, hi, halo, cap, pos, vel)
    # a neighbour's messages: the same input seen from the slabs to the left and to the right
    nl = slab_model.partition(p, lo - 2 * halo - 3, lo, halo, pos, vel, np.float32, cap=cap)
    nr = slab_model.partition(p, hi, hi + 2 * halo + 3, halo, pos, vel, np.float32, cap=cap)
    m = slab_model.partition(p, lo, hi, halo, pos, vel, np.float32, cap=cap, recv_left=nl.msg_right, recv_right=nr.msg_left)
    assert m.counts == counts and not m.overflow
    for image, (hdr, bp, bv) in ((m.msg_left, msgs[0]), (m.msg_right, msgs[1])):
        ih, ip, iv = slab_model.views(image, cap, np.float32)
        k = int(hdr[0] + hdr[1])
        assert np.array_equal(ih, hdr) and np.array_equal(bits(ip[:k]), bits(bp[:k])) and np.array_equal(bits(iv[:k]), bits(bv[:k]))
        assert not image[16 + k * 16:16 + cap * 16].any() and not image[16 + cap * 16 + k * 16:].any()   # pattern 0 elsewhere
    assert np.array_equal(bits(m.ghost_pos), bits(ghost[0])) and np.array_equal(bits(m.ghost_vel), bits(ghost[1]))
    assert np.array_equal(bits(m.stay_pos), bits(stay[0])) and np.array_equal(bits(m.stay_vel), bits(stay[1]))
    recv = [slab_model.views(im, cap, np.float32) for im in (nl.msg_right, nr.msg_left)]
    lp, lv, ln = legacy_unpack(stay, ghost, recv)
    assert m.n_owned == ln and np.array_equal(bits(m.pos), bits(lp)) and np.array_equal(bits(m.vel), bits(lv))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_partition_properties(seed, double):
    real = np.float64 if double else np.float32
    p = np.array(default_params(0), dtype=params_dtype(double)).reshape(1)
    rng = np.random.default_rng(200 + seed)
    halo = int(rng.choice([2, 8]))
    lo = int(rng.integers(-6, 10))
    hi = lo + 2 * halo + int(rng.integers(0, 5))
    n = 3000
    pos, vel = random_input(seed, n, lo, hi, halo, real, p)
    m = slab_model.partition(p, lo, hi, halo, pos, vel, real, pattern=0xA5, tail=64)
    s = {k: set(v.tolist()) for k, v in m.streams.items()}
    live = set(np.flatnonzero(pos[:, 3] == 1).tolist())
    # every live particle in exactly one of stay / migrate-left / migrate-right; nothing else anywhere
    assert s["stay"] | s["mig_l"] | s["mig_r"] == live
    assert len(s["stay"]) + len(s["mig_l"]) + len(s["mig_r"]) == len(live)
    assert s["halo_l"] <= s["stay"] and s["halo_r"] <= s["stay"] and s["ghost"] <= (s["mig_l"] | s["mig_r"])
    for v in m.streams.values():
        assert np.all(np.diff(v) > 0)   # stable slot order
    if hi - lo == 2 * halo:
        assert s["halo_l"] | s["halo_r"] == s["stay"]
    # layout: 16-byte header, pos[cap], vel[cap] in `real`, migrants first, halo copies with w = 2, pattern everywhere else
    vb, cap = 4 * np.dtype(real).itemsize, m.cap
    assert slab_model.message_bytes(cap, real) == 16 + cap * 2 * vb and len(m.msg_left) == 16 + cap * 2 * vb + 64
    for image, mig, hal in ((m.msg_left, "mig_l", "halo_l"), (m.msg_right, "mig_r", "halo_r")):
        nm, nh = len(m.streams[mig]), len(m.streams[hal])
        assert image[:16].view(np.uint32).tolist() == [nm, nh, 0, 0]
        bp = image[16:16 + (nm + nh) * vb].view(real).reshape(-1, 4)
        bv = image[16 + cap * vb:16 + cap * vb + (nm + nh) * vb].view(real).reshape(-1, 4)
        assert np.array_equal(bits(bp[:nm]), bits(pos[m.streams[mig]])) and np.all(bp[:nm, 3] == 1)
        assert np.array_equal(bits(bp[nm:, :3]), bits(pos[m.streams[hal], :3])) and np.all(bp[nm:, 3] == 2)
        assert np.array_equal(bv[:, 3], np.concatenate([m.streams[mig], m.streams[hal]]).astype(real))   # ids ride in vel.w
        assert np.all(image[16 + (nm + nh) * vb:16 + cap * vb] == 0xA5) and np.all(image[16 + cap * vb + (nm + nh) * vb:] == 0xA5)
    assert np.all(m.ghost_pos[:, 3] == 2) and np.array_equal(m.ghost_vel[:, 3], m.streams["ghost"].astype(real))


def test_missing_neighbour_and_short_buffer():
    p = default_params(0)
    pos, vel = random_input(7, 2000, 3, 9, 2, np.float32, p)
    full = slab_model.partition(p, 3, 9, 2, pos, vel, np.float32)
    end = slab_model.partition(p, 3, 9, 2, pos, vel, np.float32, left=False)
    assert end.msg_left is None and end.counts == full.counts and np.array_equal(end.msg_right, full.msg_right)
    short = slab_model.partition(p, 3, 9, 2, pos, vel, np.float32, cap=full.cap - 1, pattern=0x5A)
    assert short.overflow and not full.overflow and short.counts == full.counts
    k = full.cap - 1
    for a, b in ((short.msg_left, full.msg_left), (short.msg_right, full.msg_right)):
        (ha, pa, va), (hb, pb, vb) = slab_model.views(a, k, np.float32), slab_model.views(b, full.cap, np.float32)
        nb = min(k, int(hb[0] + hb[1]))
        assert np.array_equal(ha, hb) and np.array_equal(bits(pa[:nb]), bits(pb[:nb])) and np.array_equal(bits(va[:nb]), bits(vb[:nb]))
