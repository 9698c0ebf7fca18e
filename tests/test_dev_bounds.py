"""Guard bands and size ladders for every device-pointer entry of include/legkilo_hip.h.

The parity tests compare VALUES at realistic sizes.  This module looks at what they never see: what a kernel writes OUTSIDE the extent the
header documents (every caller-owned device buffer sits between two guard bands, tests/devguard.py), whether it leaves its INPUTS alone,
whether it writes ALL of the documented extent (outputs are pre-filled with 0xFF words), and whether the values hold at the sizes where a
tile, a wave or a workgroup ends: 1, 63, 64, 65, 255, 256, 257 items, a cloud that collapses into one voxel-grid cell, buckets of 0 / 1 /
64 points next to each other.  Every case is a few thousand points at most; the references are the CPU oracle, oracle/preprocess_oracle.py
and tests/kin_ref.py.
"""
import numpy as np
import pytest

import kin_ref
import offconfig
import preprocess_oracle as po
import scenes
from devguard import PAD, GuardError, GuardLayout, Guarded, sentinel_free, untouched
from legkilo_amd import abi, config, synth

# 64-point residual tiles, 16-byte pieces of a 4 096-byte tile block
TILE = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000]
# 256-thread kernels of the front ends, the 512-point small-bucket limit
BLOCK = [1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
# 32 messages per scatter workgroup
KIN = [1, 2, 3, 31, 32, 33, 63, 64, 65, 257]
SLOTS = [1, 2, 7, 8, 9, 63, 64, 65]
BUCKETS = [1, 63, 64, 65, 0, 128, 1, 0, 192, 257]   # sum 771; the empty ones exist only in the device's table

MAPCAPS = dict(max_roots=1 << 13, max_nodes=1 << 14, max_point_blocks=1 << 13, max_scan_points=1 << 12)   # the 10-scan map: ~8 000 root voxels
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)
PT = synth.POINT_DTYPE.itemsize
KIN_B = synth.KIN_DTYPE.itemsize
T0 = 1.0
gpu = pytest.mark.gpu


# ============================================================================ the helper's CPU self-test (no device)
@pytest.mark.parametrize("nbytes, offset, band", [(640, 16, 4096), (1, 1, 64), (0, 8, 16), (4097, 255, 4096)])
def test_guard_layout_reports_side_offset_and_count(nbytes, offset, band):
    lay = GuardLayout(nbytes, offset, band, seed=3, name="mirror")
    assert lay.total == band + PAD + nbytes + band and lay.lo == band + offset
    out = lay.image()
    assert np.all(out[lay.lo:lay.hi] == 0xFF)
    assert len(np.unique(lay.pattern)) > min(200, lay.total // 4)    # position-dependent: not one fill value
    assert lay.verify(out).size == nbytes                              # an untouched mirror passes
    # one changed byte at the first band byte, immediately before / after the payload, and at the last band byte
    for pos, side, rel in ((0, "leading", -lay.lo), (lay.lo - 1, "leading", -1), (lay.hi, "trailing", nbytes), (lay.total - 1, "trailing", lay.total - 1 - lay.lo)):
        img = out.copy()
        img[pos] ^= 0x01
        with pytest.raises(GuardError) as e:
            lay.verify(img)
        assert (e.value.side, e.value.first, e.value.last, e.value.count) == (side, rel, rel, 1), str(e.value)
        assert side in str(e.value) and f"{rel:+d}" in str(e.value)
    # a run of zeros behind the payload: first, last, count
    img = out.copy()
    k = min(24, band)
    img[lay.hi:lay.hi + k] = lay.pattern[lay.hi:lay.hi + k] ^ 0x80
    with pytest.raises(GuardError) as e:
        lay.verify(img)
    assert (e.value.side, e.value.first, e.value.last, e.value.count) == ("trailing", nbytes, nbytes + k - 1, k)
    # writing INSIDE the payload of an output is no finding
    if nbytes:
        img = out.copy()
        img[lay.lo:lay.hi] = 0
        assert not lay.verify(img).any()


def test_guard_layout_input_copy_and_sentinels():
    data = np.arange(40, dtype=np.float64)
    lay = GuardLayout(data.nbytes, 8, 128, seed=4)
    img = lay.image(data)
    assert np.array_equal(lay.verify(img).view(np.float64), data)
    img[lay.lo + 17] ^= 0xFF
    with pytest.raises(GuardError) as e:
        lay.verify(img)
    assert (e.value.side, e.value.first, e.value.last, e.value.count) == ("input", 17, 17, 1)
    with pytest.raises(AssertionError):
        lay.image(data[:-1])                    # a payload of another size
    # sentinel words: per field, in the field's own word size
    rec = np.zeros(5, dtype=synth.KIN_DTYPE)
    assert sentinel_free(rec) and sentinel_free(np.zeros(7, dtype=synth.POINT_DTYPE)) and sentinel_free(np.zeros(3, dtype=np.uint8))
    rec["contact"][3, 2] = -1
    with pytest.raises(AssertionError, match="sentinel"):
        sentinel_free(rec)
    pts = np.zeros(4, dtype=synth.POINT_DTYPE)
    pts.view(np.uint32)[9] = 0xFFFFFFFF
    with pytest.raises(AssertionError, match="sentinel"):
        sentinel_free(pts)
    assert untouched(np.full(9, 0xFF, dtype=np.uint8))
    with pytest.raises(AssertionError, match="untouched"):
        untouched(np.r_[np.full(9, 0xFF, dtype=np.uint8), np.uint8(0)])


# ============================================================================ oracle side of items 1 - 3
class Match:
    """A 10-scan oracle map and, per slot, a perturbed state with a 1 000-point cloud whose matched and unmatched points interleave."""

    def __init__(self, ob):
        self.scene = scenes.Scene(**MAPCAPS)
        self.o = ob.Oracle(self.scene.cfg(), imu_mode_only=True)
        self.blob = scenes.mature_oracle_map(self.o, self.scene, T0)
        self.o.set_map_insert(False)
        rng = np.random.default_rng(2202)
        sc = self.scene
        self.xs, self.clouds, self.valid, self.rows, self.margin = [], [], [], [], []
        self.P0 = 1e-4 * np.eye(30)
        for s in range(3):
            tb = T0 + 1.0 + 0.21 * s
            pts = synth.dense_scan(sc.world, scenes.Frozen(sc.traj, tb), tb, sc.P, n=1000, n_buckets=1, seed_scan=5100 + s)
            pts = pts[np.random.default_rng(7100 + s).permutation(len(pts))]
            x = synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5)
            self.o.set_state(x, self.P0)
            xb = scenes.xyz_of(pts)
            h, z, R, v = self.o.residuals(xb)
            self.xs.append(x), self.clouds.append(pts), self.valid.append(v), self.rows.append((h, z, R))
            self.margin.append(np.array([self.o.residual_margins(p)[1] for p in xb]))
        self.Ps = np.tile(self.P0.reshape(1, 900), (3, 1))

    def conditions(self):
        """What makes the ladder meaningful, on the oracle's side: -> (matches per slot, smallest margin)."""
        for s in range(3):
            v = self.valid[s].astype(int)
            for n in TILE:
                if n >= 31:
                    assert v[:n].sum() >= 3 and n - v[:n].sum() >= 3, (s, n, int(v[:n].sum()))
            assert self.margin[s].shape == (1000, 3) and self.margin[s].min() > 1e-6, (s, self.margin[s].min())
        return [int(v.sum()) for v in self.valid], float(min(m.min() for m in self.margin))

    def swapped(self, s, want_match):
        """Slot s's point order with the first point swapped against the first matched (unmatched) one: index array into the cloud."""
        j = int(np.flatnonzero(self.valid[s] == (1 if want_match else 0))[0])
        order = np.arange(1000)
        order[[0, j]] = order[[j, 0]]
        return order


@pytest.fixture(scope="module")
def match(oracle_lib):
    m = Match(oracle_lib)
    yield m
    m.o.close()


def test_ladder_conditions_hold_on_the_oracle(match):
    """Every prefix of 31 points or more holds at least 3 matched and 3 unmatched points, and every one of the 3 000 points sits more than
    1e-6 (relative) away from every gate on its match path: the valid mask can be required EXACT (the 100 000-point tests allow one
    rounding-level flip at margins below 1e-9)."""
    matches, margin = match.conditions()
    print(f"dev-bounds conditions: matches per slot {matches} of 1 000, smallest gate margin {margin:.3g}")


# ============================================================================ shared device helpers
def _map_handle(hip_lib, match, n_slots, kind="default", monkeypatch=None):
    """A handle holding the oracle's map.  kind "hash": created under LEGKILO_GRID=0 (roots through the hash table; the switch is read per
    handle); "negzero": ext_R = [1, -0.0, 0, ...], the generic non-identity-extrinsic instantiation with identity arithmetic;
    "classic": LEGKILO_UPDATE_CLASSIC=1 (the 256-thread update kernel)."""
    sc = offconfig.scene("negzero", **MAPCAPS) if kind == "negzero" else match.scene
    env = {"hash": ("LEGKILO_GRID", "0"), "classic": ("LEGKILO_UPDATE_CLASSIC", "1")}.get(kind)
    if env:
        monkeypatch.setenv(*env)
    try:
        g = hip_lib.LegKiloHip(sc.cfg(n_slots=n_slots))
    finally:
        if env:
            monkeypatch.delenv(env[0])
    g.map_import(match.blob)
    g.init_process_cov_q()
    return g


def _residual_rows(g, scans):
    """lk_batch_residuals_dev on len(scans) equally long scans, every caller-owned buffer guarded: -> rows8 [S, n, 8], valid [S, n]."""
    S, n = len(scans), len(scans[0])
    d_pts = Guarded.input(g, np.concatenate(scans), offset=16, name="d_pts")
    d_rows = Guarded(g, S * n * 64, offset=16, name="d_rows8")
    d_valid = Guarded(g, S * n, offset=1, name="d_valid")
    try:
        g.batch_residuals_dev(d_pts.ptr, S, n, d_rows.ptr, d_valid.ptr)
        g.synchronize()
        d_pts.check()
        rows = d_rows.read(np.float64)
        valid = d_valid.read(np.uint8)
    finally:
        for d in (d_pts, d_rows, d_valid):
            d.free()
    assert sentinel_free(rows) and sentinel_free(valid), (S, n)
    assert set(np.unique(valid).tolist()) <= {0, 1}
    return rows.reshape(S, n, 8), valid.reshape(S, n)


def _check_against_oracle(match, rows, valid):
    for s in range(3):
        ho, zo, Ro = match.rows[s]
        assert np.array_equal(valid[s], match.valid[s]), (s, np.flatnonzero(valid[s] != match.valid[s])[:8])
        h6, z, R = np.ascontiguousarray(rows[s][:, :6]), np.ascontiguousarray(rows[s][:, 6]), np.ascontiguousarray(rows[s][:, 7])
        scenes.rows_close(h6, z, R, ho, zo, Ro, match.valid[s])
        assert not rows[s][valid[s] == 0].any(), s      # records of unmatched points are all-zero


@pytest.fixture(scope="module")
def ref1000(hip_lib, match):
    """The 1 000-point, 3-slot call on a default handle, checked against the oracle: what every prefix must reproduce bit for bit."""
    match.conditions()
    g = _map_handle(hip_lib, match, 3)
    try:
        g.batch_set_priors(np.array(match.xs), match.Ps)
        rows, valid = _residual_rows(g, match.clouds)
    finally:
        g.close()
    _check_against_oracle(match, rows, valid)
    return rows, valid


# ============================================================================ 1. lk_batch_residuals_dev / lk_residuals
@gpu
@pytest.mark.parametrize("kind", ["default", "hash", "negzero"])
def test_residual_rows_size_ladder(hip_lib, match, ref1000, kind, monkeypatch):
    """A point's row depends on the point and on its slot's state - never on n_pts, on its lane or on its neighbours: for every n of the
    ladder and 1 or 3 scans, rows and valid bytes of the first n points are the first n records of the 1 000-point call, bit for bit, on
    the default handle, on the hash-table instantiation and on the generic-extrinsic one; nothing is written outside [0, n) records."""
    ref_rows, ref_valid = ref1000
    g = _map_handle(hip_lib, match, 3, kind, monkeypatch)
    try:
        g.batch_set_priors(np.array(match.xs), match.Ps)
        rows, valid = _residual_rows(g, match.clouds)
        assert np.array_equal(valid, ref_valid) and np.array_equal(rows, ref_rows), kind
        orders = [("prefix", n, [np.arange(1000)] * 3) for n in TILE]
        for n in (1, 2):   # once with a matched and once with an unmatched first point
            for want in (True, False):
                orders.append(("matched-first" if want else "unmatched-first", n, [match.swapped(s, want) for s in range(3)]))
        for name, n, order in orders:
            if name != "prefix":   # on the oracle's side
                for s in range(3):
                    assert match.valid[s][order[s][0]] == (1 if name == "matched-first" else 0)
            for S in (1, 3):
                rows, valid = _residual_rows(g, [match.clouds[s][order[s]][:n] for s in range(S)])
                for s in range(S):
                    assert np.array_equal(valid[s], ref_valid[s][order[s]][:n]), (kind, name, n, S, s)
                    assert np.array_equal(rows[s], ref_rows[s][order[s]][:n]), (kind, name, n, S, s)
            # the host entry on slot 0's state: values only
            h6, z, R, v = g.residuals(scenes.xyz_of(match.clouds[0][order[0]][:n]))
            want = ref_rows[0][order[0]][:n]
            assert np.array_equal(v, ref_valid[0][order[0]][:n]), (kind, name, n)
            assert np.array_equal(h6, want[:, :6]) and np.array_equal(z, want[:, 6]) and np.array_equal(R, want[:, 7]), (kind, name, n)
    finally:
        g.close()


# ============================================================================ 2. frozen-map batch replay at tile-edge buckets
def _bucket_scans(match, S):
    """S scans of 771 points in the bucket table BUCKETS (every non-empty bucket its own curvature).  The two 1-point buckets (points 0
    and 321) hold a point that matches deep inside its gate under the prior on even / odd slots and one that matches nothing on the
    others.  -> scans, priors, device table (offsets incl. the empty buckets, dt), per-slot N of the two 1-point buckets (oracle)."""
    sc, o = match.scene, match.o
    off = np.r_[0, np.cumsum(BUCKETS)].astype(np.uint32)
    dt = np.array([float(np.float32(0.01 * b)) for b in range(len(BUCKETS))])
    rng = np.random.default_rng(8128)
    scans, xs, ones = [], [], []
    for s in range(S):
        tb = T0 + 1.0 + 0.13 * s
        cloud = synth.dense_scan(sc.world, scenes.Frozen(sc.traj, tb), tb, sc.P, n=1000, n_buckets=1, seed_scan=5200 + s)
        cloud = cloud[np.random.default_rng(7200 + s).permutation(len(cloud))]
        x = synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5)
        o.set_state(x, match.P0)
        v = o.residuals(scenes.xyz_of(cloud))[3]
        spare = np.arange(771, 1000)
        deep = [int(i) for i in spare[v[spare] == 1] if o.residual_margins(scenes.xyz_of(cloud[i:i + 1])[0])[1].min() > 1e-3]
        miss = [int(i) for i in spare[v[spare] == 0]]
        assert len(deep) >= 2 and len(miss) >= 2, (s, len(deep), len(miss))
        scan = cloud[:771].copy()
        scan[0] = cloud[deep[0] if s % 2 == 0 else miss[0]]
        scan[321] = cloud[miss[1] if s % 2 == 0 else deep[1]]
        for b, n in enumerate(BUCKETS):
            scan["curvature"][off[b]:off[b + 1]] = np.float32(dt[b])
        o_off, o_dt = synth.buckets_of(scan)
        live = [b for b, n in enumerate(BUCKETS) if n]
        assert np.array_equal(o_off, np.r_[off[live], 771]) and np.array_equal(o_dt, dt[live])   # the oracle's bucket loop sees the same table

        def n_effect(k):
            o.set_state(x, match.P0)
            o.set_times(0.0, 0.0)
            return o.process_scan(scan[:k], 0.0)[0].n_effect if k else 0

        ones.append((n_effect(1), n_effect(322) - n_effect(321)))
        scans.append(scan), xs.append(x)
    assert off[6] == 321 and BUCKETS[0] == BUCKETS[6] == 1
    assert all(a in (0, 1) and b in (0, 1) for a, b in ones)
    assert sum(1 in p for p in ones) >= 2 and sum(0 in p for p in ones) >= 2, ones   # N == 1 and N == 0 buckets, each on two slots or more
    return scans, np.array(xs), off, dt, ones


def _oracle_replay(match, scans, xs):
    out = []
    for s, scan in enumerate(scans):
        match.o.set_state(xs[s], match.P0)
        match.o.set_times(0.0, 0.0)
        p = match.o.process_scan(scan, 0.0)[0]
        out.append(((p.n_buckets, p.n_updates, p.n_effect),) + match.o.get_state())
    return out


def _assert_replay(want, poses, states, where):
    for s, (cnt, xo, Po) in enumerate(want):
        assert cnt == (poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect), (where, s, cnt)
        xg, Pg = states[s]
        assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (where, s, np.abs(xo - xg).max())
        assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (where, s, np.abs(Po - Pg).max())


@gpu
@pytest.mark.parametrize("S", [7, 3])   # frozen-map replay (replay_groups = 3, from S = 6 on) - 7: three slot groups on three streams, split 2 / 2 / 3; 3: one stream
def test_batch_replay_tile_edge_buckets(hip_lib, match, S, monkeypatch):
    """lk_batch_replay_dev and lk_batch_replay_ragged_dev over buckets of 1, 63, 64, 65, 0, 128, 1, 0, 192, 257 points against the oracle's
    process_scan per slot (counts exact; the device's n_buckets counts the non-empty buckets, as the oracle's loop does), default and
    LEGKILO_UPDATE_CLASSIC=1 bit-identical, and d_pts - "the caller's buffer is never written" - unchanged after three replays under
    LK_BATCH_ORDER_AUTO, after lk_batch_prepare_dev and after the ragged replay."""
    scans, xs, off, dt, ones = _bucket_scans(match, S)
    print(f"S={S}: (N of bucket 0, N of bucket 6) per slot {ones}")
    want = _oracle_replay(match, scans, xs)
    assert all(w[0][0] == 8 for w in want)
    Ps = np.tile(match.P0.reshape(1, 900), (S, 1))
    allpts = np.concatenate(scans)
    first = {}
    for kind in ("default", "classic"):
        g = _map_handle(hip_lib, match, S, kind, monkeypatch)
        d_pts = Guarded.input(g, allpts, offset=16, name="d_pts")
        try:
            for rnd in range(3):   # (the third replay may read the library's voxel-ordered copy: the same scans, another order of sums)
                g.batch_set_priors(xs, Ps)
                poses = g.batch_replay_dev(d_pts.ptr, S, 771, 0.0, off, dt)
                d_pts.check()
                states = [g.get_state(slot=s) for s in range(S)]
                _assert_replay(want, poses, states, (kind, "replay", rnd))
                if rnd == 0:
                    first[kind] = ([(p.n_buckets, p.n_updates, p.n_effect) for p in poses], states)
            g.batch_changed()
            g.batch_set_priors(xs, Ps)
            g.batch_prepare_dev(d_pts.ptr, S, 771, off)
            d_pts.check()
            # the same tables through the ragged entry (empty buckets are skipped there as well)
            tables = g.ragged_tables(np.arange(S + 1) * 771, [off] * S, [dt] * S, [0.0] * S)
            g.batch_set_priors(xs, Ps)
            poses = g.batch_replay_ragged_dev(d_pts.ptr, tables)
            d_pts.check()
            _assert_replay(want, poses, [g.get_state(slot=s) for s in range(S)], (kind, "ragged"))
        finally:
            d_pts.free()
            g.close()
    assert first["default"][0] == first["classic"][0]
    for s in range(S):
        for a, b in zip(first["default"][1][s], first["classic"][1][s]):
            assert np.array_equal(a, b), s


# ============================================================================ 3. lk_batch_sort_by_voxel_dev
def _records(a):
    """16-byte records as sorted rows of two 64-bit words (a multiset)."""
    u = np.ascontiguousarray(a).view(np.uint64).reshape(-1, 2)
    return u[np.lexsort((u[:, 1], u[:, 0]))]


def _sort_case(g, scans, off):
    S, n = len(scans), len(scans[0])
    allpts = np.concatenate(scans)
    d_in = Guarded.input(g, allpts, offset=48, name="d_in")
    d_out = Guarded(g, allpts.nbytes, offset=16, name="d_out")
    try:
        g.batch_sort_by_voxel_dev(d_in.ptr, d_out.ptr, S, n, off)
        d_in.check()
        out = d_out.read(synth.POINT_DTYPE)
    finally:
        d_in.free()
        d_out.free()
    assert sentinel_free(out)
    for s in range(S):
        a, b = allpts[s * n:(s + 1) * n], out[s * n:(s + 1) * n]
        for k in range(len(off) - 1):
            lo, hi = int(off[k]), int(off[k + 1])
            assert np.array_equal(_records(a[lo:hi]), _records(b[lo:hi])), (n, s, k)   # every bucket holds exactly its own points
    return out


@gpu
def test_sort_by_voxel_tile_edge_buckets_and_ladder(hip_lib, match):
    scans, xs, off, dt, _ = _bucket_scans(match, 3)
    g = _map_handle(hip_lib, match, 3)
    try:
        g.batch_set_priors(xs, np.tile(match.P0.reshape(1, 900), (3, 1)))
        out = _sort_case(g, scans, off)
        assert not np.array_equal(out, np.concatenate(scans))     # it did sort something
        g.batch_set_priors(np.array(match.xs), match.Ps)
        for n in TILE:   # one bucket of n points
            _sort_case(g, [c[:n] for c in match.clouds], np.array([0, n], dtype=np.uint32))
    finally:
        g.close()


# ============================================================================ positive controls: the check sees a one-item overrun
def _expected_overrun(guard, item_bytes):
    """What check() must report when exactly `item_bytes` were written behind the payload: the bytes that differ from the pattern there."""
    lay = guard.lay
    item = np.frombuffer(item_bytes, dtype=np.uint8)
    diff = np.flatnonzero(item != lay.pattern[lay.hi:lay.hi + item.size])   # (a written byte equals the pattern byte at its position once in 256)
    assert diff.size >= 1
    return lay.nbytes + int(diff[0]), lay.nbytes + int(diff[-1]), int(diff.size)


@gpu
def test_positive_control_sort_overrun_is_seen(hip_lib, match):
    """The entry is called for n points while the guarded payload was declared for n - 1: the last record lands in the trailing band -
    memory of the same allocation, which really has room for it - and check() must name the trailing side and that record's bytes."""
    S, n = 3, 65
    off = np.array([0, 64, 65], dtype=np.uint32)     # a last bucket of one point: the last output record is the last input record
    scans = [c[:n] for c in match.clouds]
    allpts = np.concatenate(scans)
    g = _map_handle(hip_lib, match, S)
    d_in = Guarded.input(g, allpts, offset=48, name="d_in")
    d_out = Guarded(g, (S * n - 1) * PT, offset=16, name="d_out")
    try:
        g.batch_set_priors(np.array(match.xs), match.Ps)
        g.batch_sort_by_voxel_dev(d_in.ptr, d_out.ptr, S, n, off)
        d_in.check()
        with pytest.raises(GuardError) as e:
            d_out.check()
    finally:
        d_in.free()
        d_out.free()
        g.close()
    print("positive control (sort):", e.value)
    first, last, count = _expected_overrun(d_out, allpts[-1:].tobytes())
    assert e.value.side == "trailing" and (e.value.first, e.value.last, e.value.count) == (first, last, count), str(e.value)
    assert (S * n - 1) * PT <= e.value.first and e.value.last < S * n * PT


def _slot_states(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 36)), rng.normal(size=(n, 900))


@gpu
def test_positive_control_get_states_overrun_is_seen(hip_lib):
    n = 8
    g = hip_lib.LegKiloHip(config.make_config(config.LEG_FUSION, n_slots=65, **SMALL))
    X, P = _slot_states(65, 31)
    d_x = Guarded(g, (n - 1) * 36 * 8, offset=8, band=8192, name="d_x36")
    d_P = Guarded(g, (n - 1) * 900 * 8, offset=8, band=8192, name="d_P900")
    try:
        g.batch_set_priors(X, P)
        g.batch_get_states_dev(0, n, d_x.ptr, d_P.ptr)
        g.synchronize()
        errs = []
        for d in (d_x, d_P):
            with pytest.raises(GuardError) as e:
                d.check()
            errs.append(e.value)
    finally:
        d_x.free()
        d_P.free()
        g.close()
    for e, d, item in zip(errs, (d_x, d_P), (X[n - 1], P[n - 1])):
        print("positive control (get_states):", e)
        first, last, count = _expected_overrun(d, item.tobytes())
        assert e.side == "trailing" and (e.first, e.last, e.count) == (first, last, count), str(e)
        assert d.nbytes <= e.first and e.last < d.nbytes + item.nbytes


# ============================================================================ 4. lk_batch_get_states_dev / lk_batch_set_priors_dev
@gpu
def test_states_gather_and_priors_slot_ladder(hip_lib):
    g = hip_lib.LegKiloHip(config.make_config(config.LEG_FUSION, n_slots=65, **SMALL))
    A, PA = _slot_states(65, 41)
    B, PB = _slot_states(65, 42)
    try:
        g.batch_set_priors(A, PA)
        per_slot = [g.get_state(slot=s) for s in range(65)]
        for s in range(65):
            assert np.array_equal(per_slot[s][0], A[s]) and np.array_equal(per_slot[s][1].reshape(900), PA[s]), s
        for n in SLOTS:
            for first in (0, 3):
                if first + n > 65:
                    continue
                d_x = Guarded(g, n * 36 * 8, offset=8, name="d_x36")
                d_P = Guarded(g, n * 900 * 8, offset=8, name="d_P900")
                try:
                    g.batch_get_states_dev(first, n, d_x.ptr, d_P.ptr)
                    x, P = d_x.read(np.float64).reshape(n, 36), d_P.read(np.float64).reshape(n, 900)
                    assert sentinel_free(x) and sentinel_free(P)
                    assert np.array_equal(x, A[first:first + n]) and np.array_equal(P, PA[first:first + n]), (n, first)   # == lk_get_state, slot by slot
                    d_x.reset(), d_P.reset()
                    g.batch_get_states_dev(first, n, d_x.ptr, 0)          # d_P900 = NULL: only d_x36 is written
                    assert np.array_equal(d_x.read(np.float64).reshape(n, 36), A[first:first + n]) and untouched(d_P.check()), (n, first)
                    d_x.reset()
                    g.batch_get_states_dev(first, n, 0, d_P.ptr)          # and vice versa
                    assert np.array_equal(d_P.read(np.float64).reshape(n, 900), PA[first:first + n]) and untouched(d_x.check()), (n, first)
                finally:
                    d_x.free()
                    d_P.free()
        for n in SLOTS:   # lk_batch_set_priors_dev arms exactly slots [0, n)
            g.batch_set_priors(A, PA)
            d_x = Guarded.input(g, B[:n], offset=8, name="d_x36")
            d_P = Guarded.input(g, PB[:n], offset=8, name="d_P900")
            try:
                g.batch_set_priors_dev(d_x.ptr, d_P.ptr, n)
                d_x.check(), d_P.check()
            finally:
                d_x.free()
                d_P.free()
            x, P = g.batch_get_states(0, 65)
            assert np.array_equal(x[:n], B[:n]) and np.array_equal(P[:n].reshape(n, 900), PB[:n]), n
            assert np.array_equal(x[n:], A[n:]) and np.array_equal(P[n:].reshape(65 - n, 900), PA[n:]), n   # slot n keeps its earlier state
            xs, Ps = g.get_state(slot=n - 1)
            assert np.array_equal(xs, B[n - 1]) and np.array_equal(Ps.reshape(900), PB[n - 1])
    finally:
        g.close()


# ============================================================================ 5 - 7. the lidar front end
@pytest.fixture(scope="module")
def front_scene():
    return scenes.Scene(**SMALL)


@pytest.fixture(scope="module")
def vlp(front_scene):
    """One VLP-16 scan (curvature = time offset) with every seventh point pulled inside the 1.5 m blind radius; the first point lies outside."""
    pts = synth.vlp16_scan(front_scene.world, front_scene.traj, 2.0, front_scene.P, seed_noise=3111)
    r = np.sqrt(pts["x"].astype(np.float64) ** 2 + pts["y"].astype(np.float64) ** 2 + pts["z"].astype(np.float64) ** 2)
    near = np.arange(len(pts)) % 7 == 3
    for f in ("x", "y", "z"):
        pts[f][near] = (pts[f][near] * (1.2 / r[near])).astype(np.float32)
    assert len(pts) > 4000 and r[0] > 2.0 and r[~near].min() > 1.6
    return pts


@gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_decode_scan_dev_block_ladder(hip_lib, front_scene, vlp, lidar_type):
    """lk_decode_scan_dev: d_out has room for n_points (the header's contract) and the band behind that room stays intact; [0, n_out) and
    the two times equal the oracle's decode bit for bit.  (The tail [n_out, n_points) is the library's: not asserted.)"""
    layout, scale, stamp = synth.cloud_layout(lidar_type), synth.CLOUD_TIME_SCALE[lidar_type], 50.0
    g = hip_lib.LegKiloHip(front_scene.cfg())
    try:
        cases = [(n, fn, synth.cloud_message(vlp[:n], lidar_type, stamp, seed=n)) for n in BLOCK for fn in (1, 3)]
        near = vlp[:257].copy()       # every point but the last inside the blind radius: n_out == 1
        near["x"][:-1], near["y"][:-1], near["z"][:-1] = 0.3, -0.2, 0.1
        near["x"][-1], near["y"][-1], near["z"][-1] = 3.0, 1.0, 0.5
        cases.append((257, 1, synth.cloud_message(near, lidar_type, stamp, seed=7)))
        for n, fn, raw in cases:
            want, wb, we = po.decode(raw, lidar_type, scale, fn, 1.5, header_stamp=stamp)
            d_msg = Guarded.input(g, raw.view(np.uint8), offset=1, name="d_msg_data")
            d_out = Guarded(g, n * PT, offset=16, name="d_out")
            try:
                n_out, tb, te = g.decode_scan_dev(d_msg.ptr, n, layout, scale, fn, 1.5, stamp, d_out.ptr)
                d_msg.check()
                got = d_out.read(synth.POINT_DTYPE, n_out)
            finally:
                d_msg.free()
                d_out.free()
            assert n_out == len(want) and (tb, te) == (wb, we), (n, fn, n_out, len(want))
            assert sentinel_free(got) and got.tobytes() == want.tobytes(), (n, fn)
        assert len(want) == 1
    finally:
        g.close()


def _spread(n, leaf, rng):
    """n points, one per voxel-grid cell (a 16 x 16 x k lattice of cell centres, shuffled), 2 ms time bins."""
    i = rng.permutation(n)
    ijk = np.stack([i % 16, (i // 16) % 16, i // 256], 1).astype(np.float64)
    pts = np.zeros(n, dtype=synth.POINT_DTYPE)
    xyz = ((ijk - [8, 8, 1]) + 0.5) * leaf * 1.5 + rng.uniform(-0.1, 0.1, (n, 3)) * leaf
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["curvature"] = (rng.integers(0, 50, n) * 0.002).astype(np.float32)
    return pts


def _collapsed(n, leaf, rng):
    """n points inside one cell."""
    pts = np.zeros(n, dtype=synth.POINT_DTYPE)
    xyz = (np.array([7.0, -3.0, 2.0]) + 0.5) * leaf + rng.uniform(-0.4, 0.4, (n, 3)) * leaf
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["curvature"] = (rng.integers(0, 50, n) * 0.002).astype(np.float32)
    return pts


@gpu
def test_preprocess_scan_dev_block_ladder(hip_lib, front_scene, vlp):
    """lk_preprocess_scan_dev for n_raw of the ladder and three contents - one point per cell, all points in one cell (n_out == 1), a real
    scan's prefix: d_raw unchanged, d_out (room for n_raw) untouched behind its room, [0, n_out) equal to the oracle bit for bit."""
    leaf = 0.3
    real = synth.preprocess_velodyne(vlp, 1, 1.5)
    assert len(real) > 2000
    g = hip_lib.LegKiloHip(front_scene.cfg())
    rng = np.random.default_rng(606)
    try:
        for n in BLOCK:
            for name, raw in (("spread", _spread(n, leaf, rng)), ("collapsed", _collapsed(n, leaf, rng)), ("real", real[:n])):
                want = po.preprocess(raw, leaf)
                assert len(want) == {"spread": n, "collapsed": 1}.get(name, len(want)), (name, n, len(want))
                d_raw = Guarded.input(g, raw, offset=16, name="d_raw")
                d_out = Guarded(g, n * PT, offset=48, name="d_out_sorted")
                try:
                    n_out = g.preprocess_scan_dev(d_raw.ptr, n, leaf, d_out.ptr)
                    d_raw.check()
                    got = d_out.read(synth.POINT_DTYPE, n_out)
                finally:
                    d_raw.free()
                    d_out.free()
                assert n_out == len(want), (name, n, n_out, len(want))
                assert sentinel_free(got) and got.tobytes() == want.tobytes(), (name, n)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_decode_scans_dev_mixed_sizes(hip_lib, front_scene, vlp, lidar_type):
    """lk_decode_scans_dev over messages of 1, 257, 2, 256, 255, 1 025 and 64 points packed at odd offsets with gaps, the packed run - gaps
    included - in a guarded input at an odd and at an even device address; d_out has room for sum(n_points)."""
    sizes = [1, 257, 2, 256, 255, 1025, 64]
    layout, scale = synth.cloud_layout(lidar_type), synth.CLOUD_TIME_SCALE[lidar_type]
    stamps = 2.0 + 0.1 * np.arange(len(sizes))
    r2 = vlp["x"].astype(np.float64) ** 2 + vlp["y"].astype(np.float64) ** 2 + vlp["z"].astype(np.float64) ** 2
    starts, a = [], 0
    for n in sizes:      # every message starts at a point outside the blind radius: it keeps its first point, none decodes to nothing
        a = int(a + np.flatnonzero(r2[a:] > 4.0)[0])
        starts.append(a)
        a += n + 300
    msgs = [synth.cloud_message(vlp[a:a + n], lidar_type, float(stamps[k]), seed=40 + k) for k, (a, n) in enumerate(zip(starts, sizes))]
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=9)
    assert list(n_points) == sizes and np.all(msg_off % 2 == 1)
    want = []
    for k, raw in enumerate(msgs):
        dec, b, e = po.decode(raw, lidar_type, scale, 3, 1.5, header_stamp=float(stamps[k]))
        want.append((po.preprocess(dec, 0.3), b, e))
    g = hip_lib.LegKiloHip(front_scene.cfg())
    try:
        for offset in (1, 2):
            d_msgs = Guarded.input(g, buf, offset=offset, name="d_msgs")
            d_out = Guarded(g, sum(sizes) * PT, offset=16, name="d_out")
            try:
                so, tb, te = g.decode_scans_dev(d_msgs.ptr, msg_off, n_points, stamps, layout, scale, 3, 1.5, 0.3, d_out.ptr)
                d_msgs.check()
                got = d_out.read(synth.POINT_DTYPE, int(so[-1]))
            finally:
                d_msgs.free()
                d_out.free()
            assert sentinel_free(got)
            assert np.array_equal(so, np.r_[0, np.cumsum([len(w[0]) for w in want])]), (offset, so)
            for k, (w, b, e) in enumerate(want):
                assert got[int(so[k]):int(so[k + 1])].tobytes() == w.tobytes(), (offset, k)
                assert (tb[k], te[k]) == (b, e), (offset, k)
    finally:
        g.close()


# ============================================================================ 8. the leg kinematics front end
@gpu
@pytest.mark.parametrize("redundancy", [True, False])
def test_decode_highstate_dev_message_ladder(hip_lib, redundancy):
    """lk_decode_highstate_dev for n of the ladder, the stream at an odd device address, d_out with room for n records: records [0, n_out)
    against the restatement (bit-equal except foot position / velocity), the carried state equal afterwards; lk_kin_split_dev leaves d_kins
    as it was."""
    p = dict(config.DITER, redundancy=redundancy)
    g = hip_lib.LegKiloHip(config.make_config(p, **SMALL))
    try:
        for n in KIN:
            msgs = synth.highstate_stream(synth.Trajectory(), 2.0, 2.0 + (n + 0.5) / 500.0, p, hold=4, seed=80 + n)[0][:n]
            assert msgs.shape == (n, abi.LK_HIGHSTATE_BYTES)
            fe = kin_ref.Frontend(p)
            ref = fe.process(msgs)
            assert len(ref) == n if not redundancy else 1 <= len(ref) <= n
            g.kin_configure(p)
            d_in = Guarded.input(g, msgs, offset=1, name="d_msgs")
            d_out = Guarded(g, n * KIN_B, offset=8, name="d_out")
            try:
                k = g.decode_highstate_dev(d_in.ptr, n, d_out.ptr)
                d_in.check()
                out = d_out.read(synth.KIN_DTYPE, k)
            finally:
                d_in.free()
                d_out.free()
            assert k == len(ref), (n, k, len(ref))
            assert sentinel_free(out)
            for key in ("time_stamp", "acc", "gyr", "contact"):
                assert np.array_equal(out[key], ref[key]), (n, key)
            assert np.abs(out["foot_pos"] - ref["foot_pos"]).max() <= 1e-14 and np.abs(out["foot_vel"] - ref["foot_vel"]).max() <= 1e-12, n
            st, want = g.kin_get_frontend(), fe.state()
            assert list(st["contact"]) == list(want["contact"]) and st["last_stamp"] == want["last_stamp"], n
            assert st["last_acc_z"] == want["last_acc_z"] and st["last_gyr_z"] == want["last_gyr_z"], n
            # the kin branch of syncPackage over these records: a reader
            t = out["time_stamp"]
            ends = np.sort(np.r_[t[:: max(1, k // 5)], t[0] - 0.001, 0.5 * (t[0] + t[-1]), t[-1] + 0.001])
            d_kins = Guarded.input(g, out, offset=8, name="d_kins")
            try:
                n_msg, npk, ncs = g.kin_split_dev(d_kins.ptr, k, ends)
                d_kins.check()
            finally:
                d_kins.free()
            w_msg, w_pk, w_cs = kin_ref.sync_package(t, ends)
            assert (npk, ncs) == (w_pk, w_cs) and np.array_equal(n_msg, w_msg), (n, n_msg, w_msg)
    finally:
        g.close()


# ============================================================================ 9. the device-resident map blob
@gpu
def test_map_blob_dev_exact_size(hip_lib, match, offset=16):
    """lk_map_export_dev into a buffer of exactly the size its query gives: header | hash table | nodes | planes | blocks, the three pools
    equal to lk_map_export's sections bit for bit, the occupied hash entries equal to its root records; lk_map_import_dev reads the blob
    without changing it, gives a handle whose lk_map_export is the exporter's bit for bit, and whose re-export equals the blob."""
    g = _map_handle(hip_lib, match, 1)
    g2 = hip_lib.LegKiloHip(match.scene.cfg())
    try:
        host = g.map_export()
        hb = abi.parse_blob(host)
        size = g.map_export_dev_size()
        d_blob = Guarded(g, size, offset=offset, name="d_blob")
        d_blob2 = Guarded(g2, size, offset=offset, name="d_blob (re-export)")
        try:
            assert g.map_export_dev(d_blob.ptr, size) == size
            blob = d_blob.check()
            hd = blob[:48].view(abi.blob_header_dtype())[0]
            hh = np.frombuffer(host[:48].tobytes(), dtype=abi.blob_header_dtype())[0]
            for f in ("magic", "n_roots", "n_nodes", "n_blocks", "block_pts", "voxel_size", "max_layer", "max_points_num"):
                assert hd[f] == hh[f], f
            assert hd["version"] == (hh["version"] | 0x100) and hd["bytes"] == size and size % 256 == 0
            root_dt, node_dt, plane_dt, block_dt = abi.blob_dtypes()
            pools = int(hd["n_nodes"]) * (node_dt.itemsize + plane_dt.itemsize) + int(hd["n_blocks"]) * block_dt.itemsize
            # the hash table: 16-byte entries, a power of two of them - read off the blob's own size (less than 256 bytes of padding end it)
            hash_bytes = 1 << ((size - 48 - pools).bit_length() - 1)
            used = 48 + hash_bytes + pools
            assert used <= size < used + 256 and hash_bytes // 16 >= 2 * int(hd["n_roots"])
            assert blob[48 + hash_bytes:used].tobytes() == host[48 + int(hd["n_roots"]) * root_dt.itemsize:].tobytes()
            table = blob[48:48 + hash_bytes].view(np.int32).reshape(-1, 4)
            live = table[table[:, 3] >= 0]
            roots = np.concatenate([hb["roots"]["key"], hb["roots"]["node"][:, None]], axis=1)
            assert len(live) == len(roots) and np.array_equal(live[np.lexsort(live.T[::-1])], roots[np.lexsort(roots.T[::-1])])
            # import from the guarded blob: a reader (the second handle reads the first one's allocation: same device)
            g2.map_import_dev(d_blob.ptr, size)
            g2.synchronize()
            assert d_blob.check().tobytes() == blob.tobytes()
            assert g2.map_export().tobytes() == host.tobytes()
            assert g2.map_export_dev(d_blob2.ptr, size) == size
            assert d_blob2.check()[:used].tobytes() == blob[:used].tobytes()
        finally:
            d_blob.free()
            d_blob2.free()
    finally:
        g.close()
        g2.close()
