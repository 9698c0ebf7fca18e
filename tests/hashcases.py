"""Voxel keys chosen BY THEIR SLOT in the two open-addressing tables, and the clouds that make exactly those voxels.

The handle's root table (LkMap::hash, int4 {kx, ky, kz, node}, next_pow2(8 * max_roots) slots) and a slot's private root table of the
replays with insert (LkOverlay::keys, packed 64-bit keys) are both probed linearly from lk_hash3(key) & (cap - 1).  lk_hash3 ends in
an avalanche, so natural scenes never build a chain of more than two or three entries; here the hash is restated in numpy and the keys
of a small box are sorted by their home slot, so that a test can ask for "64 voxels in ONE chain that starts at slot 510 of 512 and
wraps past slot 0".  probe_layout is linear probing in Python: what the table must look like, and how far each key may sit from home.
"""
import numpy as np

from legkilo_amd import config, synth

# 24 x 24 x 12 = 6 912 root-voxel keys, 12 m x 12 m x 6 m at voxel_size 0.5: 25 .. 85 keys per slot of a 128-slot table, 3 .. 32 per
# slot of a 512-slot one.  x starts at 4: every point is 2 m or more from the sensor at the origin.
BOX = ((4, -12, -2), (24, 24, 12))
BOX_LOW = ((4, -12, -2), (24, 24, 6))      # its lower and upper half in z: lk_map_clear_outside drops one of them
BOX_HIGH = ((4, -12, 4), (24, 24, 6))
SPARE = ((4, 12, -2), (24, 12, 12))        # a strip beside BOX in y, for absent probe keys of a slot whose BOX keys are all in use
OUTSIDE = ((30, -12, -2), (6, 24, 12))     # keys beside BOX in x: outside the frozen grid of a base map made of BOX keys


def lk_hash3(keys):
    """lk_hash3 (lk_device.h) of (n, 3) int keys -> uint32: Teschner products, xor, three avalanche steps."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3).astype(np.uint32)      # two's complement, as (unsigned int)x
    with np.errstate(over="ignore"):
        h = (k[:, 0] * np.uint32(73856093)) ^ (k[:, 1] * np.uint32(471943)) ^ (k[:, 2] * np.uint32(83492791))
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    return h


def home_slots(cap, keys):
    assert cap & (cap - 1) == 0
    return (lk_hash3(keys) & np.uint32(cap - 1)).astype(np.int64)


def ov_pack_key(keys):
    """ov_pack_key (lk_overlay_kernels.h): three 21-bit two's complement fields, x lowest -> uint64."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    assert ((k >= -(1 << 20)) & (k < (1 << 20))).all()
    f = (k & 0x1FFFFF).astype(np.uint64)
    return f[:, 0] | (f[:, 1] << np.uint64(21)) | (f[:, 2] << np.uint64(42))


def ov_unpack_key(packed):
    p = np.asarray(packed, dtype=np.uint64).reshape(-1)
    f = np.stack([(p >> np.uint64(21 * c)) & np.uint64(0x1FFFFF) for c in range(3)], axis=1).astype(np.int64)
    return np.where(f & 0x100000, f - 0x200000, f)


def box_keys(box):
    (x0, y0, z0), (nx, ny, nz) = box
    z, y, x = np.meshgrid(np.arange(z0, z0 + nz), np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int64)


def keys_for_slots(cap, slots, box, n, exclude=()):
    """n keys of `box` whose home slot lies in `slots`, dealt round robin over the slots in the order given (a slot that runs out of
    keys is passed over), none of them in `exclude`.  Deterministic: the box is walked x fastest."""
    keys = box_keys(box)
    home = home_slots(cap, keys)
    banned = {tuple(int(v) for v in k) for k in np.asarray(exclude, dtype=np.int64).reshape(-1, 3)}
    per = [[k for k in keys[home == s] if tuple(int(v) for v in k) not in banned] for s in slots]
    out, rnd = [], 0
    while len(out) < n:
        took = False
        for lst in per:
            if rnd < len(lst) and len(out) < n:
                out.append(lst[rnd])
                took = True
        assert took, f"box {box} holds only {len(out)} keys with a home slot in {list(slots)}, {n} wanted"
        rnd += 1
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def probe_layout(cap, keys_in_order):
    """Linear probing of a cap-slot table, keys inserted in the order given -> (home, pos, dist) int arrays, one entry per key."""
    keys = np.asarray(keys_in_order, dtype=np.int64).reshape(-1, 3)
    assert len(keys) <= cap
    home = home_slots(cap, keys)
    used = np.zeros(cap, dtype=bool)
    pos = np.zeros(len(keys), dtype=np.int64)
    for i, h in enumerate(home):
        s = int(h)
        while used[s]:
            s = (s + 1) & (cap - 1)
        used[s] = True
        pos[i] = s
    return home, pos, (pos - home) & (cap - 1)


def chain_facts(cap, keys):
    """What linear probing makes of a key set WHATEVER the insertion order (the device inserts with racing threads): the occupied
    slots, and the sum of the probe distances.  The longest distance depends on the order; it lies in [dmax_lo, dmax_hi]:
    the key that ends in the chain's last slot has its home at most at the largest home offset, and a key of the smallest home
    that arrives last walks the whole chain.  `single`: the occupied slots are ONE run (start, length), so these bounds apply.
    `parities`: the distances' parities when the keys arrive sorted (the order of a blob's root records)."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    home, pos, dist = probe_layout(cap, keys)
    occ = np.zeros(cap, dtype=bool)
    occ[pos] = True
    n = len(keys)
    if n == cap:
        return dict(occupied=occ, single=True, start=0, length=cap, dist_sum=int(dist.sum()), dmax_lo=0, dmax_hi=cap - 1, full=True)
    starts = np.flatnonzero(occ & ~np.roll(occ, 1))
    start = int(starts[0])
    off = (home - start) & (cap - 1)
    return dict(occupied=occ, single=len(starts) == 1, start=start, length=n, dist_sum=int(dist.sum()),
                dmax_lo=n - 1 - int(off.max()), dmax_hi=n - 1 - int(off.min()), wraps=start + n > cap, full=False,
                parities={int(d) & 1 for d in probe_layout(cap, keys[np.lexsort(keys.T[::-1])])[2]})


def wrapping_chain(cap, n, first, n_homes=8, box=BOX, exclude=()):
    """n keys whose homes are the n_homes slots from `first` on (wrapping): one chain of n entries that starts at `first`."""
    slots = [(first + i) & (cap - 1) for i in range(n_homes)]
    return keys_for_slots(cap, slots, box, n, exclude)


def absent_probes(cap, chain_keys, box=BOX):
    """Keys that are NOT in the chain, one per home slot of interest: every slot of the chain (so the walk to the chain's end starts at
    every offset, odd and even, and wraps), the table's last slot, and the first slot behind the chain (empty at once).  Where the
    chain has used up a slot's keys of the box, the probe comes from SPARE, the strip beside it."""
    f = chain_facts(cap, chain_keys)
    want = [(f["start"] + i) & (cap - 1) for i in range(f["length"] + 1)] + [cap - 1]
    out = []
    for s in dict.fromkeys(want):
        try:
            out.append(keys_for_slots(cap, [s], box, 1, exclude=chain_keys)[0])
        except AssertionError:
            out.append(keys_for_slots(cap, [s], SPARE, 1, exclude=chain_keys)[0])
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def plane_of(key, seed):
    """The plane of a voxel as a function of its key alone (tilts a, b and the axis its normal is near): clouds made at different times
    - a base map, then the scans of a replay - put their points of one voxel on one plane."""
    rng = np.random.default_rng([int(seed)] + [int(v) & 0xFFFFFFFF for v in key])
    a, b = rng.uniform(-0.15, 0.15, 2)
    return float(a), float(b), int(rng.integers(0, 3))


def patch_points(key, voxel_size, rng, n, plane=None):
    """n points (float32 world coordinates) on a gently tilted plane with 2 mm noise, 0.1 m or more inside every face of the voxel of
    `key`: its root fits a plane (n >= layer_init_num[0] + 3), and no pose update of a test moves a point into a neighbouring voxel.
    plane: (a, b, axis) of plane_of; None: drawn from rng."""
    assert n >= 8 or plane is not None
    vs = float(voxel_size)
    assert vs >= 0.4
    lo, span = 0.1 / vs, 1.0 - 0.2 / vs                     # in-plane coordinates in voxel units: [0.2, 0.8] at 0.5 m
    uv = lo + span * rng.uniform(0, 1, (n, 2))
    if plane is None:
        a, b = rng.uniform(-0.15, 0.15, 2)
        axis = int(rng.integers(0, 3))                      # the plane's normal is near x, y or z
    else:
        a, b, axis = plane
    w = 0.5 + (a * (uv[:, 0] - 0.5) + b * (uv[:, 1] - 0.5)) + rng.normal(0, 0.002 / vs, n)
    loc = np.insert(uv, axis, w, axis=1)
    p = ((np.asarray(key, dtype=np.float64) + loc) * vs).astype(np.float32)
    k = np.floor(p.astype(np.float64) / vs).astype(np.int64)
    assert (k == np.asarray(key)).all()
    m = np.minimum(p / vs - k, k + 1 - p / vs) * vs
    assert m.min() >= 0.1 - 1e-5, m.min()
    return p


def cloud_of(keys, voxel_size, rng, per_key=10, shuffle=True):
    """patch_points of every key in one cloud (shuffled: neighbouring lanes of a launch then hold different keys AND the same key)."""
    pw = np.concatenate([patch_points(k, voxel_size, rng, per_key) for k in keys])
    if shuffle:
        rng.shuffle(pw)
    return pw


def identity_state():
    """x36 of a sensor at rest at the origin, axes along the world's."""
    x = np.zeros(36)
    x[[0, 4, 8]] = 1.0
    x[21:24] = synth.G_WORLD
    x[24:27] = -synth.G_WORLD
    return x


def body_of(pw, P=config.LEG_FUSION, x36=None):
    """The body-frame points that become pw at the pose of x36 (default: identity): world = R (E body + T) + p, as in
    test_map_build_clutter."""
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    q = np.asarray(pw, dtype=np.float64)
    if x36 is not None:
        q = (q - x36[9:12]) @ x36[:9].reshape(3, 3)
    return ((q - T) @ E).astype(np.float32)


def scan_of(pw_buckets, P=config.LEG_FUSION, dt=0.01):
    """A time-sorted scan (synth.POINT_DTYPE) whose bucket b holds the world points pw_buckets[b], seen from the identity pose."""
    out = []
    for b, pw in enumerate(pw_buckets):
        xb = body_of(pw, P)
        c = np.zeros(len(xb), dtype=synth.POINT_DTYPE)
        c["x"], c["y"], c["z"] = xb[:, 0], xb[:, 1], xb[:, 2]
        c["curvature"] = np.float32(b * dt)
        out.append(c)
    return np.concatenate(out)


def keyset(keys):
    return {tuple(int(v) for v in k) for k in np.asarray(keys).reshape(-1, 3)}


# ----------------------------------------------------------------------------- the raw table of a device blob
def device_table(g, cap):
    """The handle's root table as lk_map_export_dev holds it: (cap, 4) int32 {kx, ky, kz, node}."""
    import torch

    from legkilo_amd import abi

    nbytes = g.map_export_dev_size()
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    g.map_export_dev(d.data_ptr(), nbytes)
    hsz = abi.blob_header_dtype().itemsize
    return d[hsz: hsz + 16 * cap].cpu().numpy().view(np.int32).reshape(cap, 4).copy(), d, nbytes


def check_table(table, keys, where):
    """The invariants of linear probing on a raw root table that must hold exactly `keys`: every key once, at or behind its restated
    home slot, every slot between home and position occupied, nothing else occupied.  -> per-key probe distances (order of `keys`)."""
    cap = len(table)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    occ = table[:, 3] >= 0
    assert not (table[:, 3] == -2).any(), (where, "a slot was left locked", np.flatnonzero(table[:, 3] == -2))
    held = {}
    for s in np.flatnonzero(occ):
        k = tuple(int(v) for v in table[s, :3])
        assert k not in held, (where, "key twice in the table", k, "slots", held[k], int(s))
        held[k] = int(s)
    assert int(occ.sum()) == len(keys), (where, "occupied slots", int(occ.sum()), "roots", len(keys))
    home = home_slots(cap, keys)
    dist = np.zeros(len(keys), dtype=np.int64)
    for i, k in enumerate(keys):
        kt = tuple(int(v) for v in k)
        assert kt in held, (where, "key not in the table", kt, "home slot", int(home[i]))
        d = (held[kt] - int(home[i])) & (cap - 1)
        between = [(int(home[i]) + j) & (cap - 1) for j in range(d)]
        gaps = [s for s in between if not occ[s]]
        assert not gaps, (where, "key", kt, "home slot", int(home[i]), "found at", held[kt], "behind empty slot(s)", gaps)
        dist[i] = d
    return dist


def check_table_against_facts(table, keys, where):
    """check_table, then what no insertion order can change: the occupied slots and the sum of the distances are probe_layout's, and the
    longest distance lies inside chain_facts' bounds."""
    cap = len(table)
    dist = check_table(table, keys, where)
    f = chain_facts(cap, keys)
    occ = table[:, 3] >= 0
    assert np.array_equal(occ, f["occupied"]), (where, "occupied slots differ from linear probing's", np.flatnonzero(occ != f["occupied"]))
    assert int(dist.sum()) == f["dist_sum"], (where, "sum of probe distances", int(dist.sum()), "linear probing gives", f["dist_sum"])
    if f["single"]:
        assert f["dmax_lo"] <= int(dist.max()) <= f["dmax_hi"], (where, "longest probe distance", int(dist.max()), "allowed", f["dmax_lo"], f["dmax_hi"])
    return dist


def overlay_table(blob, cap, where):
    """A slot's private root table out of lk_overlay_export's blob, in device_table's form: a private root's node id IS its entry index."""
    from legkilo_amd import abi

    roots = abi.parse_blob(blob)["roots"]
    table = np.full((cap, 4), -1, dtype=np.int32)
    for r in roots:
        e = int(r["node"])
        assert 0 <= e < cap, (where, "private root outside the table", tuple(int(v) for v in r["key"]), "entry", e)
        assert table[e, 3] == -1, (where, "two private roots in entry", e)
        table[e] = (*[int(v) for v in r["key"]], e)
    return table
