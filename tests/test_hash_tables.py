"""The two open-addressing voxel tables on crafted collisions and at their limits (helpers: hashcases.py).

Every other test runs the handle's root table at load 0.02 .. 0.12 with chains of two or three entries.  Here the root voxels are chosen
by their home slot: 64 voxels in ONE chain that starts at slot 510 of 512 and wraps past slot 0 (part A, inside the table's contract),
and tables of 128 slots filled to a half, to 100 and to all 128 entries (part B, the limits lk_config::max_roots documents).  Every
tolerance is that of the existing test named in the docstring; lookups are exhaustive - every chain key and every absent probe key.
"""
import numpy as np
import pytest

import hashcases as hc
import scenes
from legkilo_amd import config

P = config.LEG_FUSION
VS = float(P["voxel_size"])
CAPS_A = dict(max_roots=64, max_nodes=1024, max_point_blocks=1024, max_scan_points=4096)     # table: 512 slots
CAPS_B = dict(max_roots=16, max_nodes=1024, max_point_blocks=1024, max_scan_points=4096)     # table: 128 slots, the smallest
CAP_A, CAP_B = 512, 128
FIRST_A, FIRST_B = 510, 126
QVAR = 4e-4 * np.eye(3)


def cfg(caps, **over):
    c = dict(caps)
    c.update(over)
    return config.make_config(P, **c)


def next_pow2(v):
    return 1 << max(0, int(v) - 1).bit_length()


# ----------------------------------------------------------------------------- the key sets
def keys_a():
    """64 keys, homes 510 .. 5 of 512 (eight slots, four keys each from the lower and the upper half of the box, alternating)."""
    lo = hc.wrapping_chain(CAP_A, 32, FIRST_A, 8, hc.BOX_LOW)
    hi = hc.wrapping_chain(CAP_A, 32, FIRST_A, 8, hc.BOX_HIGH)
    return np.stack([lo, hi], axis=1).reshape(-1, 3)


def keys_b(n):
    """n keys of the 128-slot table: homes 126 .. 1 (four slots) up to 100 keys - one wrapping chain; 128 keys: one per further key
    of the box in its walking order, the table is full whatever they are."""
    chain = hc.wrapping_chain(CAP_B, min(n, 100), FIRST_B, 4)
    if n <= 100:
        return chain
    have = hc.keyset(chain)
    rest = [k for k in hc.box_keys(hc.BOX) if tuple(int(v) for v in k) not in have][: n - 100]
    return np.concatenate([chain, np.array(rest)])


KEY_SETS = {
    "A: 64 of 512": (CAP_A, keys_a, 64, FIRST_A),
    "B: 64 of 128": (CAP_B, lambda: keys_b(64), 64, FIRST_B),
    "B: 65 of 128": (CAP_B, lambda: keys_b(65), 65, FIRST_B),
    "B: 100 of 128": (CAP_B, lambda: keys_b(100), 100, FIRST_B),
}


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_key_sets_are_one_wrapping_chain(name):
    """probe_layout on every chain used below: ONE chain of the stated length that starts in the table's last four slots and wraps past
    slot 0, keys at odd and at even distances from home; the absent probe keys are not in the set, there is one for every slot of the
    chain, for the slot behind it and for the table's last slot."""
    cap, make, n, first = KEY_SETS[name]
    keys = make()
    assert len(keys) == n and len(hc.keyset(keys)) == n
    f = hc.chain_facts(cap, keys)
    assert f["single"] and f["start"] == first and cap - 4 <= f["start"] and f["wraps"] and f["length"] == n, f
    assert f["parities"] == {0, 1}
    assert f["dmax_lo"] >= n - 8, f          # whatever the order, some key sits at least this far from home: far beyond a second round
    home, pos, dist = hc.probe_layout(cap, keys)
    assert sorted(pos.tolist()) == sorted(((first + np.arange(n)) & (cap - 1)).tolist())
    absent = hc.absent_probes(cap, keys)
    assert not (hc.keyset(absent) & hc.keyset(keys))
    ah = set(hc.home_slots(cap, absent).tolist())
    assert ah == {(first + i) & (cap - 1) for i in range(n + 1)} | {cap - 1}, sorted(ah)
    print(f"{name}: chain {f['start']} .. {(f['start'] + n - 1) & (cap - 1)}, load {n / cap:.3f}, longest distance within [{f['dmax_lo']}, {f['dmax_hi']}], "
          f"{len(absent)} absent probes")


def test_full_table_key_set():
    keys = keys_b(128)
    assert len(hc.keyset(keys)) == 128
    f = hc.chain_facts(CAP_B, keys)
    assert f["full"] and f["occupied"].all()
    absent = np.array([hc.keys_for_slots(CAP_B, [s], hc.BOX, 1, exclude=keys)[0] for s in range(CAP_B)])
    assert sorted(hc.home_slots(CAP_B, absent).tolist()) == list(range(CAP_B)) and not (hc.keyset(absent) & hc.keyset(keys))


def test_hash_restatement_properties():
    """The numpy restatement against what can be said without the device (the device pins it in A1): uint32 range, the packed key's
    round trip at the +-2^20 limits, and the slot statistics hashcases.BOX was sized by."""
    k = hc.box_keys(hc.BOX)
    assert len(k) == 6912
    for cap, lo, hi in ((128, 25, 85), (512, 3, 32)):
        cnt = np.bincount(hc.home_slots(cap, k), minlength=cap)
        assert lo <= cnt.min() and cnt.max() <= hi, (cap, cnt.min(), cnt.max())
    edge = np.array([[-(1 << 20), (1 << 20) - 1, 0], [-1, 1, -7], [5, -12, 9]])
    assert np.array_equal(hc.ov_unpack_key(hc.ov_pack_key(edge)), edge)
    assert hc.ov_pack_key([[1, 0, 0]])[0] == 1 and hc.ov_pack_key([[0, 1, 0]])[0] == 1 << 21 and hc.ov_pack_key([[0, 0, -1]])[0] == 0x1FFFFF << 42
    assert int(hc.lk_hash3([[0, 0, 0]])[0]) == 0


def test_table_checker_rejects_broken_tables():
    """hashcases.check_table on tables made in Python: linear probing's own layout passes; a key moved in front of its home slot (what a
    wrong wrap leaves), a key behind an empty slot (what a lost claim leaves), a key held twice (what a missed lookup makes of the next insert)
    and a slot left locked are each named."""
    keys = keys_b(64)
    home, pos, _ = hc.probe_layout(CAP_B, keys[::-1])
    good = np.full((CAP_B, 4), -1, dtype=np.int32)
    good[:, :3] = np.iinfo(np.int32).min
    for i, (k, p) in enumerate(zip(keys[::-1], pos)):
        good[p] = (*k, i)
    dist = hc.check_table_against_facts(good, keys, "good")
    assert int(dist.max()) >= 60
    t = good.copy()
    t[FIRST_B - 1], t[FIRST_B] = good[FIRST_B], good[FIRST_B - 1]
    with pytest.raises(AssertionError, match="behind empty slot"):
        hc.check_table(t, keys, "moved in front of its home")
    last = (FIRST_B + 63) & (CAP_B - 1)
    t = good.copy()
    t[(last + 2) & (CAP_B - 1)], t[last] = good[last], good[(last + 2) & (CAP_B - 1)]
    with pytest.raises(AssertionError, match="behind empty slot"):
        hc.check_table(t, keys, "behind a gap")
    t = good.copy()
    t[(last + 1) & (CAP_B - 1)] = good[FIRST_B]
    with pytest.raises(AssertionError, match="key twice in the table"):
        hc.check_table(t, keys, "twice")
    t = good.copy()
    t[(last + 1) & (CAP_B - 1), 3] = -2
    with pytest.raises(AssertionError, match="left locked"):
        hc.check_table(t, keys, "locked")
    t = good.copy()
    t[last] = good[(last + 1) & (CAP_B - 1)]
    with pytest.raises(AssertionError, match="occupied slots|not in the table"):
        hc.check_table(t, keys, "lost")


# ----------------------------------------------------------------------------- the oracle's side, computed once
class Case:
    """A key set as a cloud, the oracle's map of it, and the exhaustive query set with the oracle's answers."""

    def __init__(self, oracle_lib, caps, cap, keys, seed):
        self.caps, self.cap, self.keys = caps, cap, keys
        rng = np.random.default_rng(seed)
        self.per_key = [hc.patch_points(k, VS, rng, 10) for k in keys]
        self.pw = np.concatenate(self.per_key)
        rng.shuffle(self.pw)
        self.body = hc.body_of(self.pw)
        self.x0 = hc.identity_state()
        o = oracle_lib.Oracle(cfg(caps), imu_mode_only=True)
        o.set_state(self.x0, 1e-6 * np.eye(30))
        o.map_build(self.pw, self.body)
        self.blob = o.map_export()
        self.absent = hc.absent_probes(cap, keys) if len(keys) < cap else \
            np.array([hc.keys_for_slots(cap, [s], hc.BOX, 1, exclude=keys)[0] for s in range(cap)])
        # queries: two stored points of every chain key (2 mm off), and the centre of every absent key's voxel
        qk, qp = [], []
        for k, pts in zip(keys, self.per_key):
            for p in pts[:2]:
                qk.append(k), qp.append(p.astype(np.float64) + rng.normal(0, 0.002, 3))
        for k in self.absent:
            qk.append(k), qp.append((k + 0.5) * VS)
        self.qk, self.qp = np.array(qk, dtype=np.int32), np.array(qp)
        self.qv = np.tile(QVAR.reshape(1, 3, 3), (len(qk), 1, 1))
        self.want = [o.match_voxel(self.qk[i], self.qp[i], QVAR.reshape(9)) for i in range(len(qk))]
        self.oracle = o

    def check_match(self, g, where, exact_planes=True):
        """Every query of the set through lk_match_points against oracle.match_voxel (test_build_single_residual_per_point's
        comparisons: found / success / layer and the plane record exact, probability to 1e-9).  exact_planes=False: the handle built
        its map itself (planes equal to compare_planes' tolerance only) - flags and layer only.  -> the raw answers."""
        mg = g.match_points(self.qk, self.qp, self.qv)
        home = hc.home_slots(self.cap, self.qk)
        for i, mo in enumerate(self.want):
            tag = (where, "key", tuple(self.qk[i]), "home slot", int(home[i]))
            assert mo["found"] == bool(mg["found"][i]), tag + ("found", mo["found"], bool(mg["found"][i]))
            assert mo["success"] == bool(mg["success"][i]), tag + ("success", mo["success"])
            if mo["success"]:
                assert mo["layer"] == mg["layer"][i], tag
                if exact_planes:
                    assert np.array_equal(mo["normal"], mg["normal"][i]) and np.array_equal(mo["center"], mg["center"][i]), tag
                    assert mo["d"] == mg["d"][i], tag
                    assert np.isclose(mo["dis_to_plane"], mg["dis_to_plane"][i], rtol=1e-6, atol=1e-9), tag
                    assert np.isclose(mo["prob"], mg["prob"][i], rtol=1e-9), tag + (mo["prob"], mg["prob"][i])
            else:
                assert mg["layer"][i] == -1 and mg["prob"][i] == 0.0, tag
        return {k: np.asarray(v).tobytes() for k, v in mg.items()}


@pytest.fixture(scope="module")
def case_a(oracle_lib):
    c = Case(oracle_lib, CAPS_A, CAP_A, keys_a(), 7001)
    yield c
    c.oracle.close()


@pytest.fixture(scope="module")
def case_b64(oracle_lib):
    c = Case(oracle_lib, CAPS_B, CAP_B, keys_b(64), 7002)
    yield c
    c.oracle.close()


def oracle_preconditions(c, name):
    cm = scenes.canon_map(c.blob)
    assert set(cm) == hc.keyset(c.keys), (name, "the oracle's roots are not the crafted keys", len(cm), sorted(set(cm) ^ hc.keyset(c.keys))[:5])
    assert all(n["is_plane"] and n["layer"] == 0 for n in cm.values()), (name, "every chain key must carry a plane at its root")
    ok = {}
    for i, mo in enumerate(c.want):
        k = tuple(int(v) for v in c.qk[i])
        assert mo["found"] == (k in cm), (name, k)
        ok[k] = ok.get(k, 0) + int(mo["success"])
    none = [k for k in cm if ok[k] == 0]
    assert not none, (name, "chain keys without a matching query point", none)
    assert all(ok[tuple(int(v) for v in k)] == 0 for k in c.absent)
    return sum(ok.values())


def test_oracle_preconditions_a(case_a):
    """The oracle alone on A's cloud: exactly the 64 crafted roots, a plane on each, a matching query on each; the residual pass at
    the identity pose matches on every chain key too, and on no point of an absent voxel."""
    n_ok = oracle_preconditions(case_a, "A")
    xb, is_chain = residual_queries(case_a)
    o = case_a.oracle
    o.set_state(case_a.x0, 1e-6 * np.eye(30))
    valid = o.residuals(xb)[3].astype(bool)
    per_key = valid[is_chain].reshape(len(case_a.keys), -1).sum(1)
    assert per_key.min() > 0, ("chain keys without a valid residual", case_a.keys[per_key == 0])
    assert not valid[~is_chain].any()
    print(f"A: {n_ok} of {len(case_a.want)} voxel queries match, {int(valid.sum())} of {len(xb)} residual points valid")


def test_oracle_preconditions_b(case_b64):
    oracle_preconditions(case_b64, "B64")


def residual_queries(c):
    """Body points at the identity pose: three stored points of every chain key, and the voxel centre of every absent probe key (its
    home lookup AND its neighbour lookup walk the chain and must answer none)."""
    pw = np.concatenate([np.concatenate([p[2:5] for p in c.per_key]), ((c.absent + 0.5) * VS).astype(np.float32)])
    is_chain = np.r_[np.ones(3 * len(c.keys), bool), np.zeros(len(c.absent), bool)]
    return hc.body_of(pw), is_chain


# ----------------------------------------------------------------------------- A. inside the contract (GPU)
def new_handle(hip_lib, caps, **over):
    return hip_lib.LegKiloHip(cfg(caps, **over))


def table_report(g, keys, cap, where):
    table, d, nbytes = hc.device_table(g, cap)
    dist = hc.check_table_against_facts(table, keys, where)
    assert g.map_stats()[0] == len(keys), (where, g.map_stats())
    assert (dist & 1).any() and (~dist & 1).any(), (where, "the chain must hold keys at odd and at even distances from home")
    print(f"{where}: {len(keys)} roots in {cap} slots (load {len(keys) / cap:.3f}), probe distances read from the device table: "
          f"longest {int(dist.max())}, mean {dist.mean():.1f}, odd {int((dist & 1).sum())} / even {int((~dist & 1).sum())}")
    return table, d, nbytes


@pytest.mark.gpu
def test_a1_build_one_wrapping_chain(case_a, hip_lib):
    """lk_map_build from ONE shuffled cloud of 640 points: lanes of one launch create different keys that contend for slot 510 and
    its followers, and the same key ten times over.  The map is the oracle's (scenes.compare_maps, as test_map_build_parity); the raw
    table of lk_map_export_dev holds every root once, at or behind the home slot the numpy hash gives, with no empty slot between, and
    the distances sum to linear probing's.  Lookups on the table as the racing threads left it: every chain key found, no absent one."""
    g = new_handle(hip_lib, CAPS_A)
    try:
        g.set_state(case_a.x0, 1e-6 * np.eye(30))
        g.map_build(case_a.pw, case_a.body)
        stats = scenes.compare_maps(case_a.blob, g.map_export())
        assert stats["roots"] == 64 and stats["planes"] == 64
        table_report(g, case_a.keys, CAP_A, "A1 build")
        case_a.check_match(g, "A1 build", exact_planes=False)
    finally:
        g.close()


@pytest.mark.gpu
def test_a2_incremental_paths(case_a, oracle_lib, hip_lib):
    """The same keys through lk_map_update, eight keys a batch (test_map_update_surface's comparison after every batch), and through one
    lk_update_points bucket with insert behind a first frame of 16 of them (test_update_points_bucket_and_insert's comparisons)."""
    rng = np.random.default_rng(7003)
    o = oracle_lib.Oracle(cfg(CAPS_A), imu_mode_only=True)
    g = new_handle(hip_lib, CAPS_A)
    try:
        for b in range(0, 64, 8):
            pw = np.concatenate(case_a.per_key[b:b + 8]).astype(np.float64)
            rng.shuffle(pw)
            A = rng.normal(size=(len(pw), 3, 3)) * 0.01
            var = (A @ A.transpose(0, 2, 1) + 1e-5 * np.eye(3)).reshape(-1, 9)
            for obj in (o, g):
                obj.map_update(pw, var)
            scenes.compare_maps(o.map_export(), g.map_export())
        table_report(g, case_a.keys, CAP_A, "A2 map_update")
    finally:
        g.close()
        o.close()
    o = oracle_lib.Oracle(cfg(CAPS_A), imu_mode_only=True)
    g = new_handle(hip_lib, CAPS_A)
    try:
        first = np.concatenate(case_a.per_key[:16])
        rest = np.concatenate(case_a.per_key[16:])
        rng.shuffle(rest)
        for obj in (o, g):
            obj.set_state(case_a.x0, 1e-6 * np.eye(30))
            obj.init_process_cov_q()
            obj.set_acc_norm(9.81)
            obj.set_times(1.0, 1.0)
            obj.map_build(first, hc.body_of(first))
        wo, io_, neo = o.update_points(1.01, hc.body_of(rest))
        wg, ig, neg = g.update_points(1.01, hc.body_of(rest))
        assert neo == neg, (neo, neg)
        assert np.array_equal(io_, ig)
        assert np.abs(wo - wg).max() < 1e-5
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-10), np.abs(xg - xo).max()
        assert scenes.rel_err(Pg, Po) < 1e-7
        scenes.compare_maps(o.map_export(), g.map_export())
        table_report(g, case_a.keys, CAP_A, "A2 update_points")
    finally:
        g.close()
        o.close()


@pytest.mark.gpu
def test_a3_a4_lookups_and_rebuilds(case_a, oracle_lib, hip_lib):
    """lk_map_import of the oracle's blob - the 64 threads of lk_hash_insert_kernel all in one chain - then the table invariants and every
    query of the set through lk_match_points, exact against oracle.match_voxel.  Device export -> device import on a second handle: the
    same table bytes, the same answers bit for bit.  lk_map_clear_outside with a box that keeps z <= 3 drops every second chain key:
    the oracle's map, kept keys found and dropped ones not, the rebuilt table's invariants; re-inserting the dropped voxels
    (lk_map_update) gives the oracle's map again."""
    g = new_handle(hip_lib, CAPS_A)
    g2 = new_handle(hip_lib, CAPS_A)
    o = oracle_lib.Oracle(cfg(CAPS_A), imu_mode_only=True)
    try:
        g.map_import(case_a.blob)
        scenes.compare_maps(case_a.blob, g.map_export(), rtol=0.0)
        table, d, nbytes = table_report(g, case_a.keys, CAP_A, "A4 import")
        ans = case_a.check_match(g, "A3 import")
        g2.map_import_dev(d.data_ptr(), nbytes)
        table2, _, _ = hc.device_table(g2, CAP_A)
        assert np.array_equal(table, table2)
        assert case_a.check_match(g2, "A4 device import") == ans
        # clear outside: the low half stays
        o.map_import(case_a.blob)
        box = (100, -100, 100, -100, 3, -100)
        kept = case_a.keys[case_a.keys[:, 2] <= 3]
        dropped = case_a.keys[case_a.keys[:, 2] > 3]
        assert len(kept) == 32 and len(dropped) == 32 and np.array_equal(kept, case_a.keys[0::2])
        assert o.map_clear_outside(*box) == g.map_clear_outside(*box) == 32
        scenes.compare_maps(o.map_export(), g.map_export(), rtol=0.0)
        tbl = hc.device_table(g, CAP_A)[0]
        hc.check_table_against_facts(tbl, kept, "A4 clear_outside")
        mg = g.match_points(case_a.qk, case_a.qp, case_a.qv)
        have = hc.keyset(kept)
        home = hc.home_slots(CAP_A, case_a.qk)
        for i in range(len(case_a.qk)):
            k = tuple(int(v) for v in case_a.qk[i])
            assert bool(mg["found"][i]) == (k in have), ("A4 clear_outside", "key", k, "home slot", int(home[i]), "found", bool(mg["found"][i]))
            assert bool(mg["success"][i]) == (case_a.want[i]["success"] and k in have), ("A4 clear_outside", k)
        pw = np.concatenate(case_a.per_key[1::2]).astype(np.float64)
        var = np.tile((1e-4 * np.eye(3)).reshape(1, 9), (len(pw), 1))
        for obj in (o, g):
            obj.map_update(pw, var)
        scenes.compare_maps(o.map_export(), g.map_export())
        table_report(g, case_a.keys, CAP_A, "A4 re-insert")
    finally:
        o.close()
        g.close()
        g2.close()


def replay_inputs(c):
    """Three scans of two buckets at the identity pose for a frozen-map replay: bucket 0 stored points 2 .. 4, bucket 1 stored points 5 .. 7
    of every chain key; every bucket also holds the centre of every absent probe key's voxel.  Priors 1 cm / 0.2 deg off."""
    rng = np.random.default_rng(7004)
    ab = ((c.absent + 0.5) * VS).astype(np.float32)
    scans, xs, Ps = [], [], []
    for s in range(3):
        b0 = np.concatenate([np.concatenate([p[2:5] for p in c.per_key]), ab])
        b1 = np.concatenate([np.concatenate([p[5:8] for p in c.per_key]), ab])
        rng.shuffle(b0), rng.shuffle(b1)
        scans.append(hc.scan_of([b0, b1]))
        x = c.x0.copy()
        x[9:12] += rng.normal(0, 0.01, 3)
        a = np.deg2rad(rng.normal(0, 0.2, 3))
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        U, _, Vt = np.linalg.svd(np.eye(3) + K)
        x[:9] = (U @ Vt).reshape(-1)
        xs.append(x), Ps.append(1e-4 * np.eye(30))
    return scans, xs, Ps


@pytest.mark.gpu
def test_a3_residuals_and_frozen_replay_hash_equals_grid(case_a, hip_lib, monkeypatch):
    """lk_residuals and a frozen-map batch replay of 3 slots x 2 buckets x ~260 points, once with LEGKILO_GRID=0 (every lookup probes the
    chain) and once through the frozen-map grid: bit-identical to each other; valid mask and counts exact against the oracle, rows and
    states to test_residuals_on_imported_map's / test_frozen_grid_equals_hash_and_follows_the_map's tolerances."""
    from legkilo_amd import synth

    o = case_a.oracle
    xb, is_chain = residual_queries(case_a)
    o.set_state(case_a.x0, 1e-6 * np.eye(30))
    ho, zo, Ro, vo = o.residuals(xb)
    scans, xs, Ps = replay_inputs(case_a)
    off, dt = synth.buckets_of(scans[0])
    n_pts = len(scans[0])
    allpts = np.concatenate(scans)
    o.set_map_insert(False)
    want = []
    for s in range(3):
        o.set_state(xs[s], Ps[s])
        o.set_times(0.0, 0.0)
        po, _ = o.process_scan(scans[s], 0.0)
        want.append((po.n_buckets, po.n_updates, int(po.n_effect), o.get_state()[0].copy()))
    o.set_map_insert(True)
    assert all(w[2] > 64 for w in want), want
    res = {}
    for name, env in (("hash", "0"), ("grid", None)):
        monkeypatch.delenv("LEGKILO_GRID", raising=False)
        if env is not None:
            monkeypatch.setenv("LEGKILO_GRID", env)
        g = new_handle(hip_lib, CAPS_A, n_slots=3)
        try:
            g.map_import(case_a.blob)
            g.set_state(case_a.x0, 1e-6 * np.eye(30))
            r = g.residuals(xb)
            g.init_process_cov_q()
            d_pts = g.device_malloc(allpts.nbytes)
            g.h2d(d_pts, allpts)
            g.batch_set_priors(np.array(xs), np.array(Ps))
            poses = g.batch_replay_dev(d_pts, 3, n_pts, 0.0, off, dt)
            res[name] = (r, [(poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect), g.get_state(slot=s)[0].copy()) for s in range(3)])
            g.device_free(d_pts)
        finally:
            g.close()
    monkeypatch.delenv("LEGKILO_GRID", raising=False)
    (hg, zg, Rg, vg), rep = res["hash"]
    mism = np.flatnonzero(vo != vg)
    assert len(mism) == 0, ("valid mask differs from the oracle's at points", mism[:8])
    assert int(vg.sum()) == int(vo.sum()) and not vg[~is_chain].any()
    scenes.rows_close(hg, zg, Rg, ho, zo, Ro, vo)
    for s in range(3):
        assert rep[s][:3] == want[s][:3], (s, rep[s][:3], want[s][:3])
        assert np.allclose(rep[s][3], want[s][3], rtol=1e-8, atol=1e-9), (s, np.abs(rep[s][3] - want[s][3]).max())
    for a, b in zip(res["grid"][0], res["hash"][0]):
        assert np.array_equal(a, b), "lk_residuals: grid and hash lookups differ"
    for s in range(3):
        assert res["grid"][1][s][:3] == rep[s][:3], (s, res["grid"][1][s][:3], rep[s][:3])
        assert np.array_equal(res["grid"][1][s][3], rep[s][3]), s
    print(f"A3: {int(vo.sum())} of {len(vo)} residual points valid; replay counts {[w[:3] for w in want]}")


# ----------------------------------------------------------------------------- B. at the limits (GPU)
def built(hip_lib, keys, seed, caps=CAPS_B):
    rng = np.random.default_rng(seed)
    pw = hc.cloud_of(keys, VS, rng, 10)
    g = new_handle(hip_lib, caps)
    g.set_state(hc.identity_state(), 1e-6 * np.eye(30))
    g.map_build(pw, hc.body_of(pw))
    return g, pw


def found_flags(g, cap, keys, absent, where):
    """Every key and every absent probe through lk_match_points: found exactly for the keys."""
    q = np.concatenate([keys, absent]).astype(np.int32)
    mg = g.match_points(q, (q + 0.5) * VS, np.tile(QVAR.reshape(1, 3, 3), (len(q), 1, 1)))
    home = hc.home_slots(cap, q)
    for i in range(len(q)):
        assert bool(mg["found"][i]) == (i < len(keys)), (where, "key", tuple(q[i]), "home slot", int(home[i]), "found", bool(mg["found"][i]))


@pytest.mark.gpu
def test_b1_import_limit(case_b64, oracle_lib, hip_lib):
    """max_roots = 16, 128 slots.  The oracle's map of exactly 64 roots (hash_cap / 2, one wrapping chain) imports and every key is found;
    one of 65 roots is refused with LK_ERR_CAPACITY and the handle still holds the 64-root map, byte for byte."""
    c65 = Case(oracle_lib, CAPS_B, CAP_B, keys_b(65), 7005)
    c65.oracle.close()
    g = new_handle(hip_lib, CAPS_B)
    try:
        g.map_import(case_b64.blob)
        table_report(g, case_b64.keys, CAP_B, "B1 import of 64")
        case_b64.check_match(g, "B1 import of 64")
        before = g.map_export().tobytes()
        assert len(scenes.canon_map(c65.blob)) == 65
        with pytest.raises(hip_lib.LegKiloError, match=r"error -3: blob exceeds pool capacities"):
            g.map_import(c65.blob)
        assert g.map_export().tobytes() == before
        case_b64.check_match(g, "B1 after the refused import")
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [100, 128])
def test_b2_device_built_past_the_import_limit(oracle_lib, hip_lib, n):
    """A map BUILT on the device may hold more roots than an import accepts: at 100 of 128 slots (one chain) and at 128 of 128 (full) every
    key is found and no absent one - at 128 an absent key's lookup ends after the full circle of hash_find.  The map is the oracle's."""
    keys = keys_b(n)
    g, pw = built(hip_lib, keys, 7006 + n)
    o = oracle_lib.Oracle(cfg(CAPS_B), imu_mode_only=True)
    try:
        o.set_state(hc.identity_state(), 1e-6 * np.eye(30))
        o.map_build(pw, hc.body_of(pw))
        scenes.compare_maps(o.map_export(), g.map_export())
        table_report(g, keys, CAP_B, f"B2 build of {n}")
        absent = hc.absent_probes(CAP_B, keys) if n < CAP_B else \
            np.array([hc.keys_for_slots(CAP_B, [s], hc.BOX, 1, exclude=keys)[0] for s in range(CAP_B)])
        assert len(absent) >= n
        found_flags(g, CAP_B, keys, absent, f"B2 build of {n}")
        with pytest.raises(hip_lib.LegKiloError, match=r"error -3: blob exceeds pool capacities"):
            h2 = new_handle(hip_lib, CAPS_B)
            try:
                h2.map_import(g.map_export())        # the host export works at any count; a handle of the same max_roots refuses it
            finally:
                h2.close()
    finally:
        o.close()
        g.close()


@pytest.mark.gpu
def test_b3_full_table_refuses_loudly(case_b64, hip_lib):
    """128 roots in 128 slots, then one point in a new voxel: LK_ERR_CAPACITY whose message carries the hash bit (bits 0x1), from loops bounded
    by the table size (run once, as test_block_recycling_and_capacity_errors' refusals).  The 128 keys are still found; an import of a
    saved blob then gives a handle that answers the whole query set exactly."""
    keys = keys_b(128)
    g, _ = built(hip_lib, keys, 7134)
    try:
        extra = hc.keys_for_slots(CAP_B, [77], hc.BOX, 1, exclude=keys)[0]
        pw = hc.patch_points(extra, VS, np.random.default_rng(7135), 8).astype(np.float64)
        with pytest.raises(hip_lib.LegKiloError, match=r"error -3: device pool overflow \(bits 0x1:"):
            g.map_update(pw, np.tile((1e-4 * np.eye(3)).reshape(1, 9), (len(pw), 1)))
        found_flags(g, CAP_B, keys, extra.reshape(1, 3), "B3 full table after the refusal")
        g.map_import(case_b64.blob)
        table_report(g, case_b64.keys, CAP_B, "B3 import after the refusal")
        case_b64.check_match(g, "B3 import after the refusal")
    finally:
        g.close()


# ----------------------------------------------------------------------------- C. the overlays' private tables
CAPS_C = dict(max_roots=64, max_nodes=2048, max_point_blocks=2048, max_scan_points=4096)
OV_CAP, OV_FIRST = 128, 126          # lk_overlay_reserve(100, ..): next_pow2(100 + 25) entries; the chain's homes are slots 126, 127, 0, 1
NB, PB = 4, 384                      # buckets per scan, points per bucket (<= 512: the ragged entry runs such scans scan-resident)
PLANES = 4242                        # hashcases.plane_of's seed: one plane per voxel, whoever makes the points


def base_keys_c():
    """The base map: a 6 x 6 patch of voxels on the floor of hashcases.BOX at its low corner, and one voxel at the opposite corner - the
    frozen-map grid's box is BOX, nearly all of it empty."""
    (x0, y0, z0), (nx, ny, nz) = hc.BOX
    patch = [(x0 + i, y0 + j, z0) for j in range(6) for i in range(6)]
    return np.array(patch + [(x0 + nx - 1, y0 + ny - 1, z0 + nz - 1)], dtype=np.int64)


def overlay_key_sets():
    """Slot 0: 100 keys = 20 of the base map (copy-on-write) + a chain of 30 new keys inside the grid's box and 20 outside it, all with their
    home in slots 126, 127, 0, 1 of 128 + 15 + 15 further new keys inside / outside (any slot).  Slot 1: six keys, two of each class.
    Slot 2: slot 0's and 28 more - 128, the table exactly.  `over`: slot 2's and one more (C2)."""
    base = base_keys_c()
    cow = base[:20]
    chain_in = hc.wrapping_chain(OV_CAP, 30, OV_FIRST, 4, hc.BOX, exclude=base)
    chain_out = hc.wrapping_chain(OV_CAP, 20, OV_FIRST, 4, hc.OUTSIDE)
    used = np.concatenate([base, chain_in, chain_out])
    more_in = [k for k in hc.box_keys(hc.BOX)[::37] if tuple(int(v) for v in k) not in hc.keyset(used)][:30]
    more_out = [k for k in hc.box_keys(hc.OUTSIDE)[::11] if tuple(int(v) for v in k) not in hc.keyset(used)][:30]
    s0 = np.concatenate([cow, chain_in, chain_out, more_in[:15], more_out[:15]])
    s1 = np.concatenate([cow[:2], chain_in[:2], chain_out[:2]])
    s2 = np.concatenate([s0, more_in[15:29], more_out[15:29]])
    over = np.concatenate([s2, more_in[29:30]])
    return dict(base=base, cow=cow, chain=np.concatenate([chain_in, chain_out]), slots=[s0, s1, s2], over=over)


def scan_over(keys, seed, n_pts=NB * PB, nb=NB):
    """A scan of nb equal buckets whose n_pts points fall into exactly `keys`: every voxel's points lie on its plane_of plane and are
    dealt over the buckets, so that every bucket touches every voxel (three points or more each) - bucket 0 creates the private roots,
    bucket 1 gives them their planes, the later buckets match on them."""
    rng = np.random.default_rng(seed)
    V = len(keys)
    cnt = np.full(V, n_pts // V) + (np.arange(V) < n_pts % V)
    pw = np.concatenate([hc.patch_points(k, VS, rng, int(c), hc.plane_of(k, PLANES)) for k, c in zip(keys, cnt)])
    buckets = [pw[b::nb] for b in range(nb)]
    for b in buckets:
        rng.shuffle(b)
    return buckets


def prior(rng):
    """The identity pose, 3 mm and 0.05 degrees off (a point 15 m away moves by 16 mm: no point changes its voxel)."""
    x = hc.identity_state()
    x[9:12] += rng.normal(0, 0.003, 3)
    a = np.deg2rad(rng.normal(0, 0.05, 3))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    U, _, Vt = np.linalg.svd(np.eye(3) + K)
    x[:9] = (U @ Vt).reshape(-1)
    return x


class OverlayCase:
    """Part C's inputs and the oracle's answers, once: the base map, three scans (as one scan of four buckets, and as a run of two scans of two
    buckets), priors, and per slot the oracle's KILO::process on a private copy of the base map."""

    def __init__(self, oracle_lib):
        ks = overlay_key_sets()
        self.ks = ks
        rng = np.random.default_rng(7100)
        o = oracle_lib.Oracle(cfg(CAPS_C), imu_mode_only=True)
        self.oracle = o
        pw = np.concatenate([hc.patch_points(k, VS, rng, 10, hc.plane_of(k, PLANES)) for k in ks["base"]])
        rng.shuffle(pw)
        o.set_state(hc.identity_state(), 1e-6 * np.eye(30))
        o.map_build(pw, hc.body_of(pw))
        o.map_import(o.map_export())
        self.blob = o.map_export()
        self.base = scenes.canon_map(self.blob)
        self.buckets = [scan_over(k, 7110 + s) for s, k in enumerate(ks["slots"])]
        self.over_buckets = scan_over(ks["over"], 7119)
        self.scans = [hc.scan_of(b) for b in self.buckets]
        self.runs = [[hc.scan_of(b[:2]), hc.scan_of(b[2:])] for b in self.buckets]
        self.run_tbs = [[0.0, 0.05]] * 3
        self.xs = [prior(rng) for _ in range(3)]
        self.Ps = [1e-4 * np.eye(30)] * 3
        self.want_scan = [self.oracle_run(s, [self.scans[s]], [0.0]) for s in range(3)]
        self.want_runs = [self.oracle_run(s, self.runs[s], self.run_tbs[s]) for s in range(3)]

    def oracle_run(self, s, scans, tbs):
        o = self.oracle
        o.map_import(self.blob)
        o.set_map_insert(True)
        o.init_process_cov_q()
        o.set_state(self.xs[s], self.Ps[s])
        o.set_times(tbs[0], tbs[0])
        counts = []
        for pts, tb in zip(scans, tbs):
            po, _ = o.process_scan(pts, tb)
            counts.append((po.n_buckets, po.n_updates, int(po.n_effect)))
        x, Pm = o.get_state()
        return dict(counts=counts, x=x.copy(), P=Pm.copy(), after=scenes.canon_map(o.map_export()))

    def private_keys(self, want):
        return {k for k, n in want["after"].items() if k not in self.base or scenes.subtree_sig(n) != scenes.subtree_sig(self.base[k])}


@pytest.fixture(scope="module")
def case_c(oracle_lib):
    c = OverlayCase(oracle_lib)
    yield c
    c.oracle.close()


def test_overlay_key_sets():
    """probe_layout on the overlay key sets (128 entries): slot 0 holds 100 distinct keys (load 0.78) of three classes, 50 of them with their
    home in slots 126 .. 1, so the run of occupied entries through slot 126 wraps and is 50 or longer; slot 2 holds 128; C2's 129."""
    ks = overlay_key_sets()
    base, (s0, s1, s2) = hc.keyset(ks["base"]), ks["slots"]
    assert [len(hc.keyset(k)) for k in (s0, s1, s2, ks["over"])] == [100, 6, 128, 129]
    (x0, y0, z0), (nx, ny, nz) = hc.BOX
    lo, hi = ks["base"].min(0), ks["base"].max(0)
    assert tuple(lo) == (x0, y0, z0) and tuple(hi) == (x0 + nx - 1, y0 + ny - 1, z0 + nz - 1), "the base map's key box must be BOX"
    for name, keys in (("slot 0", s0), ("slot 1", s1), ("slot 2", s2)):
        inbox = ((keys >= lo) & (keys <= hi)).all(1)
        cow = np.array([tuple(int(v) for v in k) in base for k in keys])
        assert cow.sum() >= 2 and (inbox & ~cow).sum() >= 2 and (~inbox).sum() >= 2, (name, "needs keys of all three classes")
    assert set(hc.home_slots(OV_CAP, ks["chain"]).tolist()) == {126, 127, 0, 1} and len(ks["chain"]) == 50
    home, pos, dist = hc.probe_layout(OV_CAP, s0)
    occ = np.zeros(OV_CAP, bool)
    occ[pos] = True
    run = 0
    while occ[(OV_FIRST + run) & (OV_CAP - 1)] and run < OV_CAP:
        run += 1
    assert run >= 50 and OV_FIRST + run > OV_CAP, run
    chain_dist = dist[np.isin(home, [126, 127, 0, 1])]
    assert {int(d) & 1 for d in chain_dist} == {0, 1} and chain_dist.max() >= 40
    print(f"overlay slot 0: 100 keys in 128 entries (load {100 / 128:.2f}), run through entry 126: {run} entries, longest distance {int(dist.max())} in this order")


def test_oracle_preconditions_c(case_c):
    """The oracle alone on part C's scans, as one scan and as a run of two: per slot it changes or creates exactly the intended voxels, every
    bucket updates, and the later buckets match on the slot's own voxels (more matches than the base map's voxels could give)."""
    for form, wants in (("scan", case_c.want_scan), ("runs", case_c.want_runs)):
        for s, w in enumerate(wants):
            keys = hc.keyset(case_c.ks["slots"][s])
            got = case_c.private_keys(w)
            assert got == keys, (form, s, "voxels the oracle changed are not the crafted keys", sorted(got ^ keys)[:6])
            assert sum(c[0] for c in w["counts"]) == NB and sum(c[1] for c in w["counts"]) == NB, (form, s, w["counts"])
            n_eff = sum(c[2] for c in w["counts"])
            cow = sum(1 for k in keys if k in case_c.base)
            assert n_eff > 0, (form, s)
            print(f"C oracle {form} slot {s}: {len(keys)} voxels ({cow} copy-on-write), counts {w['counts']}")
        assert sum(c[2] for c in wants[0]["counts"]) > 2 * PB, "slot 0's later buckets must match on private voxels"


def overlay_handle(hip_lib, c, reserve=(100, 1024, 1024)):
    g = new_handle(hip_lib, CAPS_C, n_slots=3)
    g.map_import(c.blob)
    g.init_process_cov_q()
    if reserve:
        g.overlay_reserve(*reserve)
    return g


def check_overlay_slots(g, c, wants, counts, where):
    """Per slot against the oracle (test_batch_replay_overlay's comparisons and tolerances): counts exact, state 1e-6, covariance 1e-6 of its
    largest entry, the private voxels of lk_overlay_export equal to the oracle's; and the slot's private table - exactly the crafted keys,
    each at or behind its home entry with no empty entry between.  -> (states, covariances, exports)."""
    X, Pm = g.batch_get_states(0, 3)
    exports = [g.overlay_export(s) for s in range(3)]
    cap = g.overlay_pool_bytes()[1]
    assert cap == OV_CAP, (where, g.overlay_pool_bytes())
    for s, w in enumerate(wants):
        assert counts[s] == w["counts"], (where, "slot", s, counts[s], w["counts"])
        assert np.abs(w["x"] - X[s]).max() < 1e-6, (where, "slot", s, np.abs(w["x"] - X[s]).max())
        assert np.abs(Pm[s] - w["P"]).max() <= 1e-6 * np.abs(w["P"]).max(), (where, "slot", s)
        st = scenes.compare_overlay(exports[s], c.base, w["after"], (where, s), rtol=1e-5, ptol=1e-7)
        keys = c.ks["slots"][s]
        assert st["private_roots"] == st["changed_roots"] == len(keys), (where, "slot", s, st)
        dist = hc.check_table_against_facts(hc.overlay_table(exports[s], cap, (where, "slot", s)), keys, (where, "slot", s))
        print(f"{where} slot {s}: {len(keys)} private roots in {cap} entries (load {len(keys) / cap:.2f}), distances read from the device table: "
              f"longest {int(dist.max())}, mean {dist.mean():.1f}; counts {counts[s]}, max |dx| {np.abs(w['x'] - X[s]).max():.1e}")
    return X, Pm, exports


def pose_counts(poses):
    return [(p.n_buckets, p.n_updates, int(p.n_effect)) for p in poses]


@pytest.mark.gpu
def test_c1_c2_uniform_entry_chains_and_overflow(case_c, hip_lib):
    """lk_batch_replay_overlay_dev under lk_overlay_reserve(100, ..) - 128 entries per slot.  Slot 0 touches 100 voxels (load 0.78, 50 of them
    with their home in entries 126 .. 1: copy-on-write keys, new keys inside the base grid's box, keys outside it), slot 1 six, slot 2 exactly
    128; four buckets, so that buckets 1 .. 3 find their voxels - and miss their neighbours - through the chains bucket 0 built.  C2: the same
    reserve with a 129-voxel scan in slot 0 is LK_ERR_CAPACITY "overlay pool overflow" with bit 1, the slots stay at their priors, and the handle
    replays C1 to C1's bits."""
    import re

    from legkilo_amd import synth

    c = case_c
    off, dt = synth.buckets_of(c.scans[0])
    assert all(np.array_equal(synth.buckets_of(sc)[0], off) for sc in c.scans)
    g = overlay_handle(hip_lib, c)
    try:
        g.batch_set_priors(np.array(c.xs), np.array(c.Ps))
        poses = g.batch_replay_overlay(c.scans, 0.0, off, dt)
        X, Pm, exports = check_overlay_slots(g, c, c.want_scan, [[pc] for pc in pose_counts(poses)], "C1 uniform")
        assert scenes.maps_identical(g.map_export(), c.blob) == len(c.base)         # the handle's map is untouched
        over = [hc.scan_of(c.over_buckets), c.scans[1], c.scans[2]]
        g.batch_set_priors(np.array(c.xs), np.array(c.Ps))
        Xp, Pp = g.batch_get_states(0, 3)
        with pytest.raises(hip_lib.LegKiloError, match=r"error -3: overlay pool overflow in slot 0 \(bits 0x") as ei:
            g.batch_replay_overlay(over, 0.0, off, dt)
        bits = int(re.search(r"bits 0x([0-9a-f]+)", str(ei.value)).group(1), 16)
        assert bits & 1, str(ei.value)
        Xa, Pa = g.batch_get_states(0, 3)
        assert np.array_equal(Xa, Xp) and np.array_equal(Pa, Pp), "a refused replay must leave the slots at their priors"
        g.batch_set_priors(np.array(c.xs), np.array(c.Ps))
        poses2 = g.batch_replay_overlay(c.scans, 0.0, off, dt)
        X2, P2 = g.batch_get_states(0, 3)
        assert pose_counts(poses2) == pose_counts(poses) and np.array_equal(X2, X) and np.array_equal(P2, Pm)
        for s in range(3):
            assert scenes.maps_identical(g.overlay_export(s), exports[s]), s
    finally:
        g.close()


@pytest.mark.gpu
def test_c1_ragged_entry_resident_and_launch_by_launch(case_c, hip_lib, monkeypatch):
    """The same scans through lk_batch_replay_overlay_ragged_dev, scan-resident (every bucket holds 384 points) and launch by launch
    (LEGKILO_RAG_RESIDENT=0): each equal to the oracle, the two bit-identical - states, covariances, counts, every private voxel."""
    c = case_c
    res = {}
    for name, env in (("resident", None), ("launches", "0")):
        monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
        if env is not None:
            monkeypatch.setenv("LEGKILO_RAG_RESIDENT", env)
        g = overlay_handle(hip_lib, c)
        try:
            poses = g.batch_replay_overlay_ragged(c.scans, [0.0] * 3, c.xs, c.Ps)
            rounds = g.overlay_resident_rounds()
            assert (rounds > 0) == (env is None), (name, rounds)
            res[name] = (pose_counts(poses),) + check_overlay_slots(g, c, c.want_scan, [[pc] for pc in pose_counts(poses)], f"C1 ragged {name}")
        finally:
            g.close()
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    a, b = res["resident"], res["launches"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "scan-resident and launch-by-launch replay differ"
    for s in range(3):
        assert scenes.maps_identical(a[3][s], b[3][s]), s


@pytest.mark.gpu
def test_c1_runs_entry_second_scan_starts_on_private_roots(case_c, hip_lib):
    """lk_batch_replay_overlay_runs_dev, every slot a run of two scans of two buckets: the second scan's first lookups already go through the
    private table the first scan filled.  Per scan the counts, per run the final state and the private voxels are the oracle's."""
    c = case_c
    g = overlay_handle(hip_lib, c)
    try:
        poses = g.batch_replay_overlay_runs(c.runs, c.run_tbs, c.xs, c.Ps)
        check_overlay_slots(g, c, c.want_runs, [pose_counts(run) for run in poses], "C1 runs")
    finally:
        g.close()


@pytest.mark.gpu
def test_a4_overlay_commit_extends_the_chain(case_a, oracle_lib, hip_lib):
    """lk_overlay_commit: the base map holds 40 keys of part A's chain, one slot's scan touches four of them and the other 24 - the commit's
    rebuild of the handle's table (lk_hash_insert_kernel over base and private roots) puts all 64 into the one chain from slot 510.  The
    committed map equals the oracle's after KILO::process of that scan (compare_maps at test_batch_replay_overlay's tolerances)."""
    from legkilo_amd import synth

    keys = case_a.keys
    rng = np.random.default_rng(7200)
    pw = np.concatenate([hc.patch_points(k, VS, rng, 10, hc.plane_of(k, PLANES)) for k in keys[:40]])
    rng.shuffle(pw)
    buckets = scan_over(np.concatenate([keys[:4], keys[40:]]), 7201, n_pts=4 * 112, nb=4)
    scan = hc.scan_of(buckets)
    x = prior(rng)
    o = oracle_lib.Oracle(cfg(CAPS_A), imu_mode_only=True)
    g = new_handle(hip_lib, CAPS_A)
    try:
        o.set_state(hc.identity_state(), 1e-6 * np.eye(30))
        o.map_build(pw, hc.body_of(pw))
        o.map_import(o.map_export())
        blob = o.map_export()
        o.init_process_cov_q()
        o.set_state(x, 1e-4 * np.eye(30))
        o.set_times(0.0, 0.0)
        po, _ = o.process_scan(scan, 0.0)
        g.map_import(blob)
        g.init_process_cov_q()
        table_report(g, keys[:40], CAP_A, "A4 commit: base")
        g.batch_set_priors(x.reshape(1, 36), (1e-4 * np.eye(30)).reshape(1, 900))
        off, dt = synth.buckets_of(scan)
        poses = g.batch_replay_overlay([scan], 0.0, off, dt)
        assert pose_counts(poses) == [(po.n_buckets, po.n_updates, int(po.n_effect))]
        g.overlay_commit(0)
        st = scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-7)
        assert st["roots"] == 64
        table_report(g, keys, CAP_A, "A4 commit: committed")
        found_flags(g, CAP_A, keys, case_a.absent, "A4 commit: committed")
    finally:
        g.close()
        o.close()


# ----------------------------------------------------------------------------- C3. growth by doubling
N3, NB3 = 4400, 2        # points per scan, buckets: the same for the three replays, or the history rule does not apply


def c3_keys(n):
    """n keys of BOX and OUTSIDE in walking order, every third: no slot is chosen here, only the count matters."""
    return np.concatenate([hc.box_keys(hc.BOX), hc.box_keys(hc.OUTSIDE)])[::3][:n]


def c3_replay(g, scan):
    from legkilo_amd import synth

    off, dt = synth.buckets_of(scan)
    x = hc.identity_state()
    g.batch_set_priors(x.reshape(1, 36), (1e-4 * np.eye(30)).reshape(1, 900))
    poses = g.batch_replay_overlay([scan], 0.0, off, dt)
    X, Pm = g.batch_get_states(0, 1)
    return pose_counts(poses), X, Pm


@pytest.mark.gpu
def test_c3_library_sized_pools_grow_by_doubling(case_c, hip_lib):
    """Pools the library sizes itself (no lk_overlay_reserve), one slot, 4 400 points per scan in two buckets.
    A scan over 10 voxels, twice: the first replay's pools are the first guess (roots = min(max(2048, n / 18), max(1024, n)) = 2048, table 4096),
    the second's follow the history rule on its high-water marks (ov_reserve): roots = hw + hw / 4 + 64 = 76 at hw = 10, table =
    next_pow2(76 + 19) = 128, blocks = hwb + hwb / 4 + 64 - the first guess is more than twice that and is replaced (asserted through
    lk_overlay_pool_bytes, as test_overlay_pool_capacities does).
    Then a scan over 600 voxels.  ov_attempt_end lets attempts 0 .. 3 grow what overflowed and run again, so a table grows by 2^4 at most:
    128 -> 256 -> 512 -> 1024 holds 600 keys after THREE doublings (512 < 600), 2048 would be the last.  A scan that cannot claim its roots
    reports the table alone - what the missing roots need is never asked for - so ov_reserve lets blocks and child nodes follow a doubled
    table in the first guess's proportions: roots = 4/5 of the entries, a block per root, a child node per two.  At 1024 entries that is
    1024 / 5 * 4 = 816 blocks (600 voxels of 7 points need one each) and 408 child nodes, and the fourth attempt fits.  (This test found the rule missing:
    the table took three of the four growth attempts, the blocks, 76 from the history rule, doubled once to 152, and the replay failed with
    LK_ERR_CAPACITY on pools the caller had never sized.)  The result is bit-equal to a fresh handle's under an ample explicit reserve.
    Between the two, from the same 128 entries, a scan over 2 200 voxels: more than 2048, the table after four doublings.  The header says
    what then happens (lk_overlay_reserve): LK_ERR_CAPACITY "overlay pool overflow", the slot back at its prior, the handle usable - the
    600-voxel replay behind it starts from the history rule's pools again (the refused scan left no high-water marks), and the 10-voxel scan
    replays to its first bits at the end."""
    small = hc.scan_of(scan_over(c3_keys(10), 7300, N3, NB3))
    big_keys = c3_keys(600)
    big = hc.scan_of(scan_over(big_keys, 7301, N3, NB3))
    huge = hc.scan_of(scan_over(c3_keys(2200), 7302, N3, NB3))
    g = new_handle(hip_lib, CAPS_C, n_slots=1)
    ref = new_handle(hip_lib, CAPS_C, n_slots=1)
    try:
        for h in (g, ref):
            h.map_import(case_c.blob)
            h.init_process_cov_q()
        first = c3_replay(g, small)
        assert g.overlay_pool_bytes()[1] == 4096, g.overlay_pool_bytes()
        hw_roots, hw_nodes, hw_blocks = g.overlay_stats()
        assert hw_roots == 10
        second = c3_replay(g, small)
        roots = hw_roots + hw_roots // 4 + 64
        child = max(hw_nodes - hw_roots, 0)
        shrunk = (next_pow2(roots + roots // 4), child + child // 4 + 256, hw_blocks + hw_blocks // 4 + 64)
        print("C3 pools after the history rule:", g.overlay_pool_bytes(), "high-water marks", (hw_roots, hw_nodes, hw_blocks))
        assert shrunk[0] == 128 and g.overlay_pool_bytes()[1:] == shrunk
        assert second[0] == first[0] and np.array_equal(second[1], first[1]) and np.array_equal(second[2], first[2])
        x = hc.identity_state()
        with pytest.raises(hip_lib.LegKiloError, match=r"error -3: overlay pool overflow in slot 0 \(bits 0x"):
            c3_replay(g, huge)
        Xa, Pa = g.batch_get_states(0, 1)
        assert np.array_equal(Xa[0], x) and np.array_equal(Pa[0], 1e-4 * np.eye(30)), "a refused replay must leave the slot at its prior"
        print("C3 pools after the refused 2 200-voxel scan:", g.overlay_pool_bytes())
        assert g.overlay_pool_bytes()[1] == 2048
        third = c3_replay(g, big)
        hw3 = g.overlay_stats()
        caps = g.overlay_pool_bytes()[1:]
        print("C3 pools after the 600-voxel scan:", g.overlay_pool_bytes(), "high-water marks", hw3)
        assert hw3[0] == 600
        table, nodes, blocks, doublings = shrunk[0], shrunk[1], shrunk[2], 0
        while table < 600:          # an attempt whose table overflows: the table doubles and takes the first guess's proportions with it
            table *= 2
            blocks, nodes, doublings = max(blocks, table // 5 * 4), max(nodes, table // 5 * 4 // 2), doublings + 1
        assert doublings == 3 and blocks >= hw3[2] and nodes >= hw3[1] - hw3[0], (table, nodes, blocks, hw3)
        assert caps == (table, nodes, blocks) == (1024, 408, 816), (caps, shrunk, hw3)
        hd = hc.check_table_against_facts(hc.overlay_table(g.overlay_export(0), caps[0], "C3"), big_keys, "C3 grown table")
        print(f"C3 grown table: 600 keys in 1024 entries, longest distance read from the device table {int(hd.max())}")
        ref.overlay_reserve(1024, 4096, 2048)
        want = c3_replay(ref, big)
        assert third[0] == want[0] and np.array_equal(third[1], want[1]) and np.array_equal(third[2], want[2])
        assert scenes.maps_identical(g.overlay_export(0), ref.overlay_export(0)) == 600
        again = c3_replay(g, small)
        assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    finally:
        g.close()
        ref.close()
