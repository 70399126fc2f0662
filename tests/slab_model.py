"""A plain numpy statement of nrs_slab_pack / nrs_slab_unpack (include/nereus_hip.h, nereus_amd/csrc/nrs_kernels_slab.h) for either
precision: which slot goes into which of the six streams, in which order, with which w tag, at which byte of the message.

Test infrastructure only.  It is the one statement of the partition that the gloo protocol tests (tests/slab_check_engine.py) and the
device tests (tests/test_slab_partition_gpu.py) share.  Everything is slot order in, stable slot order out; all arithmetic is in
`real`, the cell-x comes from nereus_amd.slab.cell_of.  Only w == 1 is live: entries with w of 2 (last step's halo / ghost copies), 0
or NaN are dropped.  Live particles with a non-finite x are not a defined input (the float-to-integer conversion of a NaN differs
between host and device): callers leave them out.
"""
import numpy as np

from nereus_amd.slab import cell_of

STREAMS = ("stay", "mig_l", "halo_l", "mig_r", "halo_r", "ghost")   # the order of nrs_slab_pack's counts[6]
HEADER_BYTES = 16


def message_bytes(cap, real):
    """nrs_slab_message_bytes: [u32 nMigrants, u32 nHalo, u32 0, u32 0 | vec4 pos[cap] | vec4 vel[cap]]"""
    return HEADER_BYTES + int(cap) * 2 * 4 * np.dtype(real).itemsize


def classify(params, lo, hi, halo, pos, real):
    """the six streams as index arrays into `pos`, each in ascending (= stable) slot order"""
    pos = np.asarray(pos, real).reshape(-1, 4)
    ox, cs = params["worldOrigin"][0][0], params["cellSize"][0][0]
    live = np.flatnonzero(pos[:, 3] == real(1))       # (NaN compares false)
    cx = cell_of(pos[live, 0], ox, cs, real=real)
    lo, hi, halo = int(lo), int(hi), int(halo)
    stay = (cx >= lo) & (cx < hi)
    mig_l, mig_r = cx < lo, cx >= hi
    masks = dict(stay=stay, mig_l=mig_l, halo_l=stay & (cx < lo + halo), mig_r=mig_r, halo_r=stay & (cx >= hi - halo),
                 ghost=(mig_l & (cx >= lo - halo)) | (mig_r & (cx < hi + halo)))
    return {k: live[masks[k]] for k in STREAMS}


def _tag(a, real):
    a = a.copy()
    a[:, 3] = real(2)   # read-only copy
    return a


def views(image, cap, real):
    """(header u32[4], pos (cap, 4), vel (cap, 4)) as views of a message image (np.uint8, at least message_bytes(cap) long)"""
    vb = 4 * np.dtype(real).itemsize
    hdr = image[:HEADER_BYTES].view(np.uint32)
    bp = image[HEADER_BYTES:HEADER_BYTES + cap * vb].view(real).reshape(cap, 4)
    bv = image[HEADER_BYTES + cap * vb:HEADER_BYTES + 2 * cap * vb].view(real).reshape(cap, 4)
    return hdr, bp, bv


def message_image(mig_pos, mig_vel, halo_pos, halo_vel, cap, real, pattern=0, tail=0):
    """One message, byte for byte: header with the two stream populations, migrants first, then halo copies tagged w = 2.  Entries at
    or beyond `cap` are not written (the header still holds the populations: the receiver refuses it).  Every byte that the pack
    does not write, the `tail` bytes behind the message included, holds `pattern`."""
    image = np.full(message_bytes(cap, real) + int(tail), pattern, np.uint8)
    hdr, bp, bv = views(image, cap, real)
    nm, nh = len(mig_pos), len(halo_pos)
    hdr[:] = (nm, nh, 0, 0)
    allp = np.concatenate([np.asarray(mig_pos, real).reshape(-1, 4), _tag(np.asarray(halo_pos, real).reshape(-1, 4), real)])
    allv = np.concatenate([np.asarray(mig_vel, real).reshape(-1, 4), np.asarray(halo_vel, real).reshape(-1, 4)])
    k = min(nm + nh, cap)
    bp[:k], bv[:k] = allp[:k], allv[:k]
    return image


class Partition:
    """what partition() returns (plain attributes)"""


def partition(params, lo, hi, halo, pos, vel, real, cap=None, left=True, right=True, pattern=0, tail=0,
              recv_left=None, recv_right=None):
    """nrs_slab_pack (and, with received messages, nrs_slab_unpack) of the arrays pos, vel (slot order) for the slab [lo, hi).

    cap: particles per message buffer (None: as many as the fuller side needs, at least 1).  left / right: whether that neighbour
    exists (False = the NULL pointer at an end of the chain: no image; the counts still report who left).  pattern / tail: see
    message_image.  Returns a Partition with
      streams     {name: indices}         counts      [stay, mig_l, halo_l, mig_r, halo_r, ghost]
      msg_left / msg_right                np.uint8 images (None for a missing neighbour)
      ghost_pos / ghost_vel               our read-only copies of fresh migrants (w = 2), at most cap of them
      stay_pos / stay_vel                 the compacted owned particles
      overflow                            a message or the ghost array does not fit cap (NRS_E_CAPACITY)
    and, when recv_left / recv_right are given (images or None), the arrays after the unpack: pos, vel, n_owned (see unpack)."""
    pos = np.ascontiguousarray(pos, real).reshape(-1, 4)
    vel = np.ascontiguousarray(vel, real).reshape(-1, 4)
    s = classify(params, lo, hi, halo, pos, real)
    r = Partition()
    r.real, r.streams = real, s
    r.counts = [int(len(s[k])) for k in STREAMS]
    need = max(len(s["mig_l"]) + len(s["halo_l"]), len(s["mig_r"]) + len(s["halo_r"]))
    r.cap = cap = max(1, need) if cap is None else int(cap)
    r.msg_left = message_image(pos[s["mig_l"]], vel[s["mig_l"]], pos[s["halo_l"]], vel[s["halo_l"]], cap, real, pattern, tail) if left else None
    r.msg_right = message_image(pos[s["mig_r"]], vel[s["mig_r"]], pos[s["halo_r"]], vel[s["halo_r"]], cap, real, pattern, tail) if right else None
    r.ghost_pos, r.ghost_vel = _tag(pos[s["ghost"]], real)[:cap], vel[s["ghost"]][:cap]
    r.stay_pos, r.stay_vel = pos[s["stay"]], vel[s["stay"]]
    r.overflow = need > cap or len(s["ghost"]) > cap
    if recv_left is not None or recv_right is not None:
        r.pos, r.vel, r.n_owned = unpack(r, recv_left, recv_right)
    return r


def unpack_arrays(stay_pos, stay_vel, ghost_pos, ghost_vel, recv_left, recv_right, cap, real):
    """nrs_slab_unpack: (pos, vel, n_owned) in the order [stay | migrants left | migrants right | ghosts | halo left | halo right];
    the first n_owned are owned.  recv_*: message images of capacity `cap`, or None."""
    mig_p, mig_v, hal_p, hal_v = [], [], [], []
    for image in (recv_left, recv_right):
        if image is None:
            continue
        hdr, bp, bv = views(image, cap, real)
        nm, nh = int(hdr[0]), int(hdr[1])
        assert nm + nh <= cap, "corrupt slab message header"
        mig_p.append(bp[:nm].copy()); mig_v.append(bv[:nm].copy())
        hal_p.append(bp[nm:nm + nh].copy()); hal_v.append(bv[nm:nm + nh].copy())
    n_owned = len(stay_pos) + sum(len(a) for a in mig_p)
    pos = np.concatenate([stay_pos] + mig_p + [ghost_pos] + hal_p)
    vel = np.concatenate([stay_vel] + mig_v + [ghost_vel] + hal_v)
    return pos, vel, n_owned


def unpack(part, recv_left, recv_right):
    """unpack_arrays behind the Partition `part`"""
    return unpack_arrays(part.stay_pos, part.stay_vel, part.ghost_pos, part.ghost_vel, recv_left, recv_right, part.cap, part.real)


def random_input(seed, n, lo, hi, halo, real, params):
    """x random over [lo - halo - 2, hi + halo + 2) cells, a third of the entries with w in {2, 0, NaN}, plus every cut face and the
    halo faces with nextafter in both directions; ids in vel.w"""
    rng = np.random.default_rng(seed)
    ox, cs = real(params["worldOrigin"][0][0]), real(params["cellSize"][0][0])
    pos = np.empty((n, 4), real)
    pos[:, 0] = (ox + cs * rng.uniform(lo - halo - 2, hi + halo + 2, n)).astype(real)
    pos[:, 1:3] = rng.uniform(0.1, 0.9, (n, 2)).astype(real)
    faces = []
    for k in (lo - halo, lo, lo + halo, hi - halo, hi, hi + halo):
        f = real(ox + real(k) * cs)
        faces += [f, np.nextafter(f, real(-np.inf)), np.nextafter(f, real(np.inf))]
    m = min(n, len(faces))
    at = rng.choice(n, m, replace=False)
    pos[at, 0] = np.array(faces, real)[:m]
    w = np.ones(n, real)
    dead = rng.random(n) < 1.0 / 3.0
    w[dead] = rng.choice(np.array([2.0, 0.0, np.nan], real), int(dead.sum()))
    w[at] = 1
    pos[:, 3] = w
    vel = rng.normal(0, 1, (n, 4)).astype(real)
    vel[:, 3] = np.arange(n)
    return pos, vel
