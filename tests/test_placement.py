"""-m gpu parity AWAY from the origin, at the size limits of the frozen-map grid and past the packed-key range of the overlay.

Every other parity test runs in one room centred on the origin (tests/placement.py): nothing there takes the world transform, the key
arithmetic, the matcher's n.p + (double)d, the raw-moment plane fit or the float range gate to coordinates of 10^2 .. 10^3 m, to all-
negative keys, or to walls off the voxel faces.  tests/test_placement_pin.py pins the oracle against the reference at the same
placements, which makes it the checker here - for what holds there: OPEN-loop parity (a common map blob, common priors, one call) is
exact at every placement and carries the project's tolerances WITHOUT their rtol (1e-8 relative of a 3 km position would be 3e-5 m);
closed-loop parity with those tolerances holds at `origin` and `negz` only, because the reference's own plane refit loses eps |p|^2
("Parity away from the origin").  Plane fits are judged against a long-double fit of the same points with the rounding
bound B of placement.plane_fit_errors; device against device, identities that hold by design hold bit for bit at any placement.

Sizes: caps of test_range_gate_ladder.py; the oracle's map of a first frame + 4 VLP-16 scans, imported; scans of 6 000 points in 3
buckets; 6 slots (the three slot groups run).
"""
import numpy as np
import pytest

import offconfig
import placement
import scenes
import test_config_space as tcs
from legkilo_amd import abi, synth
from test_range_gate_ladder import CAPS

pytestmark = pytest.mark.gpu

S, N_PTS, NB = 6, 6000, 3
T0 = 1.0
OPEN_LOOP = ("negz", "neg", "far")
LK_ERR_INVALID, LK_ERR_STATE = -1, -5
_cache = {}


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def placed_map(place, oracle_lib):
    """(scene, map blob, state, covariance, last time) of an oracle after the first frame + 4 config-1 scans at the placement, once per module run."""
    if ("map", place) not in _cache:
        sc = placement.placed_scene(place, **CAPS)
        o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
        blob = bytes(scenes.mature_oracle_map(o, sc, T0, n_scans=4))
        xs, Ps = o.get_state()
        _cache[("map", place)] = (sc, blob, xs, Ps, o.get_times()[0])
        o.close()
    return _cache[("map", place)]


def batch_of(sc, tp, seed=5005):
    """S equally shaped scans (N_PTS points in NB buckets, z = 0 forced on every 37th point) with perturbed priors, as test_batch_replay_frozen_map draws them."""
    rng = np.random.default_rng(seed)
    xs, Ps, scans = [], [], []
    for s in range(S):
        tb = tp + 0.2 + 0.37 * s
        pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=N_PTS, n_buckets=NB, seed_scan=seed + s, seed_noise=seed + 1001 + s)
        pts["z"][::37] = 0.0
        scans.append(pts)
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
    return scans, xs, Ps


def ready(obj, blob):
    obj.map_import(u8(blob))
    obj.init_process_cov_q()
    obj.set_acc_norm(9.81)
    return obj


def oracle_frozen(o, scans, tbs, xs, Ps, imus=None):
    """The oracle's bucket loop with insert off over each scan alone -> [(n_buckets, n_updates, n_effect, x, P)]."""
    o.set_map_insert(False)
    out = []
    for s in range(len(scans)):
        o.set_state(xs[s], Ps[s])
        o.set_times(tbs[s], tbs[s])
        po, _ = o.process_scan(scans[s], tbs[s], **({} if imus is None else dict(imus=imus[s])))
        x, P = o.get_state()
        out.append((po.n_buckets, po.n_updates, int(po.n_effect), x.copy(), P.copy()))
    return out


def grab(g, poses):
    n = len(poses)
    X, P = g.batch_get_states(0, n)
    return [(poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect), X[s].copy(), P[s].copy()) for s in range(n)]


def same_bits(a, b, where):
    assert len(a) == len(b), where
    for s, (ra, rb) in enumerate(zip(a, b)):
        assert ra[:3] == rb[:3], (where, s, ra[:3], rb[:3])
        assert np.array_equal(ra[3], rb[3]) and np.array_equal(ra[4], rb[4]), (where, s, np.abs(ra[3] - rb[3]).max())


def check_abs(want, got, where, least_effect=0):
    """Counts exact; every state component within 1e-8 ABSOLUTE, position included (the project's tolerance of the frozen replay without
    its rtol); covariance 1e-6 of its largest entry.  -> largest state difference."""
    worst = 0.0
    for s, (w, r) in enumerate(zip(want, got)):
        assert w[:3] == r[:3], (where, s, w[:3], r[:3])
        assert w[2] > least_effect, (where, s, w[2])
        d = float(np.abs(w[3] - r[3]).max())
        worst = max(worst, d)
        assert d <= 1e-8, (where, s, d, int(np.abs(w[3] - r[3]).argmax()))
        assert np.abs(w[4] - r[4]).max() <= 1e-6 * np.abs(w[4]).max(), (where, s)
    return worst


# ============================================================================= 3a. build and insert
def same_tree_and_points(blob_a, blob_b):
    """Equal root key sets, tree shape, counters, state bits, is_plane and geometry; stored world points bit-equal (their variances to the
    1e-7 of scenes.compare_nodes: lk_map_build derives them on the device).  Plane records are judged by plane_fit_errors instead."""
    A, B = scenes.canon_map(blob_a), scenes.canon_map(blob_b)
    assert set(A) == set(B), ("root key sets differ", len(A), len(B), sorted(set(A) ^ set(B))[:5])
    keep = abi.LK_NODE_INIT_OCTO | abi.LK_NODE_UPDATE_ENABLE | abi.LK_NODE_OCTO_STATE | abi.LK_NODE_PTS_DROPPED
    n = [0, 0]

    def same(a, b, where):
        for f in ("layer", "npts", "new_points", "is_plane", "quater"):
            assert a[f] == b[f], (where, f, a[f], b[f])
        assert (a["state"] & keep) == (b["state"] & keep), (where, "state", a["state"], b["state"])
        assert np.array_equal(a["center"], b["center"]), (where, "voxel centre")
        if a["is_plane"]:
            assert a["plane"]["points_size"] == b["plane"]["points_size"], (where, "points_size")
            n[1] += 1
        assert (a["pts"] is None) == (b["pts"] is None), (where, "points presence")
        if a["pts"] is not None:
            assert np.array_equal(a["pts"]["pw"], b["pts"]["pw"]), (where, "stored points")
            sc_ = np.abs(a["pts"]["var"]).max() + 1e-300
            assert np.abs(a["pts"]["var"] - b["pts"]["var"]).max() <= 1e-7 * sc_, (where, "stored variances")
        assert set(a["children"]) == set(b["children"]), (where, "children")
        n[0] += 1
        for c in a["children"]:
            same(a["children"][c], b["children"][c], where + (c,))

    for k in A:
        same(A[k], B[k], (k,))
    return len(A), n[0], n[1]


def check_fits(blob, where, least=1):
    en, ec, B = placement.plane_fit_errors(blob)
    assert len(en) >= least, (where, len(en))
    ratio = float(np.max(en / B))
    print(f"{where}: {len(en)} planes against their long-double fit: max normal error / B {ratio:.3f} (p99 {np.quantile(en / B, 0.99):.3f}), max centre error {ec.max():.2e} m")
    assert (en <= 1.0 * B).all(), (where, ratio)
    assert ec.max() <= 1e-9, (where, float(ec.max()))
    return ratio


@pytest.mark.parametrize("place", OPEN_LOOP)
def test_build_and_insert(oracle_lib, hip_lib, place):
    """lk_map_build of a dense first frame, then lk_map_update of one further scan's world points in chunks of 1, 1, 5, 17, 200, 1 000,
    5 000, rest - key_trunc / key_floor at negative and large keys, dev_init_plane's raw moments at |p| up to 3.6 km.  Against the
    oracle fed the same arrays: same voxels, tree, counters, state bits, is_plane, stored points, after the build and after every chunk;
    every device plane within 1.0 x B (normal) and 1e-9 m (centre) of the long-double fit of its own stored points; at `negz`, where
    the fit conditions as at the origin, scenes.compare_maps at its default tolerances as well.
    Measured on an MI355X (negz / neg / far): largest normal error / B 0.094 / 0.080 / 0.078 over 768 / 793 / 821 planes - the oracle's
    figures to three digits -, largest centre error 1.5e-15 / 6.9e-15 / 2.1e-13 m."""
    sc = placement.placed_scene(place, **CAPS)
    o, g = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True), hip_lib.LegKiloHip(sc.cfg())
    for obj in (o, g):
        x0 = scenes.init_filter(obj, sc, T0)
        scenes.first_frame(obj, sc, T0, x0, dense=20000)
    roots, nodes, planes = same_tree_and_points(o.map_export(), g.map_export())
    assert roots > 1000 and planes > 500, (roots, planes)
    check_fits(g.map_export(), f"{place} lk_map_build", least=500)
    tb = T0 + 0.1
    xb = scenes.xyz_of(scenes.vlp_scan_input(sc, tb, 1))
    pw = scenes.world_of(synth.initial_state(sc.traj, tb, sc.P), xb, sc.P).astype(np.float64)
    var = np.tile((np.eye(3) * 4e-4).reshape(1, 9), (len(pw), 1))
    for a, b in offconfig.chunks_of(len(pw)):
        for obj in (o, g):
            obj.map_update(pw[a:b], var[a:b])
        same_tree_and_points(o.map_export(), g.map_export())
    blob_g = g.map_export()
    assert len(scenes.canon_map(blob_g)) > roots, "the scan must have created voxels"
    ratio = check_fits(blob_g, f"{place} lk_map_update", least=500)
    check_fits(o.map_export(), f"{place} oracle", least=500)
    if place == "negz":
        print(place, scenes.compare_maps(o.map_export(), blob_g))
    print(f"{place}: {len(pw)} points inserted, largest normal error / B on the device {ratio:.3f}")
    tcs.close(g, o)


# ============================================================================= 3b. rows and matcher, open loop
def batch_rows(g, scans, xs, Ps):
    n = len(scans) * N_PTS
    allpts = np.concatenate(scans)
    d_pts, d_rows, d_v = g.device_malloc(allpts.nbytes), g.device_malloc(n * 64), g.device_malloc(n)
    g.h2d(d_pts, allpts)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    g.batch_residuals_dev(d_pts, len(scans), N_PTS, d_rows, d_v)
    g.synchronize()
    rows8, v = np.zeros((n, 8)), np.zeros(n, dtype=np.uint8)
    g.d2h(rows8, d_rows)
    g.d2h(v, d_v)
    for d in (d_pts, d_rows, d_v):
        g.device_free(d)
    return rows8, v


@pytest.mark.parametrize("place", OPEN_LOOP)
def test_rows_and_matcher_open_loop(oracle_lib, hip_lib, monkeypatch, place):
    """lk_residuals, lk_batch_residuals_dev and lk_match_points on the imported blob against the oracle: masks by the flip rule of
    check_mask_and_rows (max_flips=1), rows by rows_close at its present tolerances, the matcher's decisions exact.  The batch entry in
    its default form (frozen-map grid, kernel specialised for ext_R == I), with the generic kernel and with LEGKILO_GRID=0: the same bits.
    LEGKILO_XID is read once per process, so setting it here selects the generic kernel only in a process that has not launched a
    residual kernel before; the handle created with -0.0 in ext_R (offconfig `negzero`) takes the generic kernel whatever ran before.
    Measured on an MI355X (negz / neg / far): 11 410 / 12 254 / 12 440 of 36 000 rows valid, no mask flip; 275 / 285 / 264 matcher successes."""
    sc, blob, xs0, Ps0, tp = placed_map(place, oracle_lib)
    scans, xs, Ps = batch_of(sc, tp, seed=2202)
    o = ready(oracle_lib.Oracle(sc.cfg(n_slots=S), imu_mode_only=True), blob)
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), blob)
    rows8, v = batch_rows(g, scans, xs, Ps)
    monkeypatch.setenv("LEGKILO_XID", "0")
    forms = dict(xid0=hip_lib.LegKiloHip(sc.cfg(n_slots=S)),
                 generic=hip_lib.LegKiloHip(placement.placed_scene(place, "negzero", **CAPS).cfg(n_slots=S)))
    for name, gf in forms.items():
        r2, v2 = batch_rows(ready(gf, blob), scans, xs, Ps)
        assert np.array_equal(v2, v) and np.array_equal(r2, rows8), (place, name)
    monkeypatch.delenv("LEGKILO_XID")
    g0 = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), blob)
    r2, v2 = batch_rows(g0, scans, xs, Ps)
    assert np.array_equal(v2, v) and np.array_equal(r2, rows8), (place, "LEGKILO_GRID=0")
    h6, z, R = np.ascontiguousarray(rows8[:, :6]), np.ascontiguousarray(rows8[:, 6]), np.ascontiguousarray(rows8[:, 7])
    n_valid = n_flips = 0
    for s in range(S):
        a, b = s * N_PTS, (s + 1) * N_PTS
        xb = scenes.xyz_of(scans[s])
        o.set_state(xs[s], Ps[s])
        ro = o.residuals(xb)
        n_valid += int(ro[3].sum())
        n_flips += tcs.check_mask_and_rows(o, f"{place} slot {s}", xb, ro, (h6[a:b], z[a:b], R[a:b], v[a:b]), max_flips=1)
        unm = v[a:b] == 0
        assert not h6[a:b][unm].any() and not z[a:b][unm].any() and not R[a:b][unm].any()
        g.set_state(xs[s], Ps[s], slot=0)    # the host entry: the same bits
        hh, zh, Rh, vh = g.residuals(xb)
        assert np.array_equal(vh, v[a:b]) and np.array_equal(hh, h6[a:b]) and np.array_equal(zh, z[a:b]) and np.array_equal(Rh, R[a:b]), s
    print(f"{place}: {n_valid} of {S * N_PTS} rows valid, {n_flips} flips")
    assert n_valid >= 1500 and n_flips <= 1, (n_valid, n_flips)
    # ---- the matcher: caller-held world points on their home voxel and one neighbour
    rng = np.random.default_rng(41)
    pw = scenes.world_of(xs[0], scenes.xyz_of(scans[0])[:600], sc.P).astype(np.float64) + rng.normal(0, 0.02, (600, 3))
    vs = float(sc.P["voxel_size"])
    keys, Pq, V = [], [], []
    for i, p in enumerate(pw):
        k0 = oracle_lib.key_floor(p, vs)
        A = rng.normal(size=(3, 3))
        var = (A @ A.T) * (1e-5 if i % 3 else 4e-3) + np.eye(3) * 1e-6
        for dk in ((0, 0, 0), (0, -1, 0)):
            keys.append([a_ + b_ for a_, b_ in zip(k0, dk)]), Pq.append(p), V.append(var)
    per_layer, n_found = tcs.match_points_against_oracle(o, g, oracle_lib, np.array(keys, dtype=np.int32), np.array(Pq), np.array(V))
    print(f"{place}: lk_match_points found {n_found} of {len(keys)}, successes per layer {per_layer}")
    assert n_found > 600 and sum(per_layer.values()) > 200, (n_found, per_layer)
    tcs.close(g0, *forms.values(), g, o)


# ============================================================================= 3c. frozen-map replay, open loop
def uniform_entries(g, scans, xs, Ps):
    """The equally shaped batch through lk_batch_replay_dev (as given, and in its default form: the voxel-ordered copy),
    lk_batch_replay_ragged_dev and lk_batch_replay_scans_dev."""
    off, dt = synth.buckets_of(scans[0])
    for s_ in scans:
        o2, d2 = synth.buckets_of(s_)
        assert np.array_equal(o2, off) and np.array_equal(d2, dt)
    allpts = np.concatenate(scans)
    so = np.arange(S + 1) * N_PTS
    d_pts = g.device_malloc(allpts.nbytes)
    g.h2d(d_pts, allpts)
    out = {}
    X, P = np.array(xs), np.array(Ps)
    g.batch_order(0)
    g.batch_set_priors(X, P)
    out["uniform"] = grab(g, g.batch_replay_dev(d_pts, S, N_PTS, 0.0, off, dt))
    g.batch_set_priors(X, P)
    out["ragged"] = grab(g, g.batch_replay_ragged_dev(d_pts, g.ragged_tables(so, [off] * S, [dt] * S, [0.0] * S)))
    g.batch_set_priors(X, P)
    out["scans"] = grab(g, g.batch_replay_scans_dev(d_pts, so, [0.0] * S))
    g.batch_order(1)
    g.batch_set_priors(X, P)
    out["ordered"] = grab(g, g.batch_replay_dev(d_pts, S, N_PTS, 0.0, off, dt))
    g.device_free(d_pts)
    return out


def config1_batch(sc, tp):
    """S config-1 scans (hundreds of 2 ms buckets of a dozen points: the scan-wave kernel's shape) with perturbed priors and their IMU messages."""
    rng = np.random.default_rng(8118)
    scans, tbs, xs, Ps, imus = [], [], [], [], []
    for s in range(S):
        tb = tp + 0.1 + 0.23 * s
        scans.append(scenes.vlp_scan_input(sc, tb, 40 + s))
        tbs.append(tb)
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
        imus.append(synth.imu_stream(sc.traj, tb, tb + 0.1, seed=8600 + s))
    return scans, tbs, xs, Ps, imus


def ragged_entries(g, scans, tbs, xs, Ps, imus, monkeypatch):
    """The config-1 batch through lk_batch_replay_ragged_dev - one wave per scan, and bucket by bucket (LEGKILO_RAGGED_LEVELS=1) - and
    lk_batch_replay_scans_dev, then with the IMU messages between the buckets."""
    out = {}
    monkeypatch.delenv("LEGKILO_RAGGED_LEVELS", raising=False)
    out["scan-wave"] = grab(g, g.batch_replay_ragged(scans, tbs, xs, Ps, host_tables=True))
    monkeypatch.setenv("LEGKILO_RAGGED_LEVELS", "1")
    out["levels"] = grab(g, g.batch_replay_ragged(scans, tbs, xs, Ps, host_tables=True))
    monkeypatch.delenv("LEGKILO_RAGGED_LEVELS")
    out["scans"] = grab(g, g.batch_replay_ragged(scans, tbs, xs, Ps))
    out["imu"] = grab(g, g.batch_replay_ragged(scans, tbs, xs, Ps, imus=imus, host_tables=True))
    out["imu-scans"] = grab(g, g.batch_replay_ragged(scans, tbs, xs, Ps, imus=imus))
    return out


@pytest.mark.parametrize("place", OPEN_LOOP)
def test_frozen_replay_open_loop(oracle_lib, hip_lib, monkeypatch, place):
    """lk_batch_replay_dev, lk_batch_replay_ragged_dev (one wave per scan, and LEGKILO_RAGGED_LEVELS=1) and lk_batch_replay_scans_dev on
    the imported blob, each on the frozen-map grid and with LEGKILO_GRID=0.  Bit-identical where the suite asserts it at the origin:
    grid = hash for every entry; on the batch as given uniform = ragged = device-built tables; one wave per scan = bucket by bucket =
    device-built tables, with and without IMU messages.  Against the oracle's bucket loop with insert off: counts equal, every state
    component within 1e-8 absolute, covariance 1e-6.
    Measured on an MI355X, largest |x_device - x_oracle| over all entries: negz 2.9e-13, neg 8.7e-13, far 9.0e-13."""
    sc, blob, xs0, Ps0, tp = placed_map(place, oracle_lib)
    o = ready(oracle_lib.Oracle(sc.cfg(), imu_mode_only=True), blob)
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), blob)
    g0 = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), blob)
    scans, xs, Ps = batch_of(sc, tp)
    uni, uni0 = uniform_entries(g, scans, xs, Ps), uniform_entries(g0, scans, xs, Ps)
    for name in uni:
        same_bits(uni[name], uni0[name], (place, name, "grid vs LEGKILO_GRID=0"))
    same_bits(uni["uniform"], uni["ragged"], (place, "uniform vs ragged"))
    same_bits(uni["ragged"], uni["scans"], (place, "ragged vs device-built tables"))
    want = oracle_frozen(o, scans, [0.0] * S, xs, Ps)
    worst = max(check_abs(want, uni[name], (place, name), least_effect=300) for name in ("uniform", "ordered"))
    c1 = config1_batch(sc, tp)
    rag, rag0 = ragged_entries(g, *c1, monkeypatch), ragged_entries(g0, *c1, monkeypatch)
    for name in rag:
        same_bits(rag[name], rag0[name], (place, name, "grid vs LEGKILO_GRID=0"))
    same_bits(rag["scan-wave"], rag["levels"], (place, "one wave per scan vs bucket by bucket"))
    same_bits(rag["scan-wave"], rag["scans"], (place, "host tables vs device-built tables"))
    same_bits(rag["imu"], rag["imu-scans"], (place, "IMU: host tables vs device-built tables"))
    scans1, tbs1, xs1, Ps1, imus1 = c1
    worst = max(worst, check_abs(oracle_frozen(o, scans1, tbs1, xs1, Ps1), rag["scan-wave"], (place, "config-1"), least_effect=300))
    o.set_acc_norm(9.81)
    worst = max(worst, check_abs(oracle_frozen(o, scans1, tbs1, xs1, Ps1, imus=imus1), rag["imu"], (place, "config-1 + IMU"), least_effect=300))
    print(f"{place}: frozen replay, largest |x_device - x_oracle| over all entries {worst:.2e}")
    tcs.close(g0, g, o)


# ============================================================================= 3g. slide and clear
@pytest.mark.parametrize("place", ["neg", "far"])
def test_slide_and_clear_on_the_imported_blob(oracle_lib, hip_lib, place):
    """lk_map_slide with a position two thresholds from the last slide and lk_map_clear_outside with a box through the map, at keys
    around -200 and +-6 000: the same voxels leave as in the oracle, what remains is the same map bit for bit, the pools are compacted to
    it (test_map_sliding_parity_and_compaction) - and a frozen replay on the compacted pools equals the oracle's (measured 1.0e-14 / 1.2e-14)."""
    sc, blob, xs0, Ps0, tp = placed_map(place, oracle_lib)
    o = ready(oracle_lib.Oracle(sc.cfg(), imu_mode_only=True), blob)
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), blob)
    roots0, nodes0, blocks0 = g.map_stats()
    pos = np.array(xs0[9:12])
    thresh = 4.0
    for obj in (o, g):
        obj.set_last_slide_position(pos)
        assert obj.map_slide(pos + [0.5 * thresh, 0.0, 0.0], thresh, 16) == (False, 0)
    so, sg = o.map_slide(pos + [2 * thresh, 0.0, 0.0], thresh, 16), g.map_slide(pos + [2 * thresh, 0.0, 0.0], thresh, 16)
    assert so == sg and sg[0] and 0 < sg[1] < roots0, (so, sg, roots0)
    assert np.array_equal(g.get_last_slide_position(), o.get_last_slide_position())
    blob_g = g.map_export()
    assert scenes.maps_identical(o.map_export(), blob_g) == roots0 - sg[1]
    roots1, nodes1, blocks1 = g.map_stats()
    assert roots1 == roots0 - sg[1] and (nodes1, blocks1) == tcs.count_tree(blob_g) and nodes1 < nodes0
    k = np.floor(pos / float(np.float32(sc.P["voxel_size"]))).astype(int)
    box = (k[0] + 20, k[0] + 3, k[1] + 9, k[1] - 12, k[2] + 8, k[2] - 8)
    co, cg = o.map_clear_outside(*box), g.map_clear_outside(*box)
    assert co == cg and 0 < cg < roots1, (co, cg, roots1)
    blob_g = g.map_export()
    left = scenes.maps_identical(o.map_export(), blob_g)
    assert g.map_stats() == (left,) + tcs.count_tree(blob_g) and left == roots1 - cg
    print(f"{place}: {roots0} roots, {sg[1]} slid out, {cg} cleared, {left} left")
    scans, xs, Ps = batch_of(sc, tp)
    poses, X, Pc = tcs.frozen_replay(g, scans, xs, Ps)
    got = [(poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect), X[s], Pc[s].reshape(30, 30)) for s in range(S)]
    worst = check_abs(oracle_frozen(o, scans, [0.0] * S, xs, Ps), got, (place, "after slide and clear"), least_effect=100)
    print(f"{place}: frozen replay on the compacted pools, largest |x_device - x_oracle| {worst:.2e}")
    tcs.close(g, o)


# ============================================================================= 4. the size limits of the frozen-map grid
GRID_DIMS = (256, 256, 250)     # 16 384 000 cells: in (0.95 * 2^24, 2^24]; the room's key box (82 x 62 x 19) lies in its corner
N_PATCH, N_ON_PATCH = 3000, 300


def key_box(blob):
    keys = abi.parse_blob(blob)["roots"]["key"].astype(np.int64)
    return keys.min(0), keys.max(0) - keys.min(0) + 1


def patch_points(key, vs, seed, n, noise):
    """n points on a tilted plane, `noise` across it, 0.3 m wide, strictly inside the voxel of `key`."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    u = np.cross(nrm, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    w = np.cross(nrm, u)
    ab = rng.uniform(-0.15, 0.15, (n, 2))
    p = (np.asarray(key, float) + 0.5) * vs + ab[:, :1] * u + ab[:, 1:] * w + rng.normal(0, noise, (n, 1)) * nrm
    assert np.all(np.floor(p / vs) == np.asarray(key)), "the patch must stay inside its voxel"
    return p


def grid_limit_case(oracle_lib, dz_extra):
    """The origin's map + a patch in the voxel kmin + GRID_DIMS - 1 (+ dz_extra voxels in z): the patch owns the LAST cell of a grid of
    GRID_DIMS (dz_extra = 0) or pushes the key box over kGridMaxCells (dz_extra = 8).  -> dict(sc, base blob, blob, patch key, cells,
    scans, xs, Ps); bucket 0 of slot 0 begins with N_ON_PATCH points on the patch, and slot 0's prior stands 3 m from it."""
    key = ("limit", dz_extra)
    if key in _cache:
        return _cache[key]
    sc, base, xs0, Ps0, tp = placed_map("origin", oracle_lib)
    vs = float(sc.P["voxel_size"])
    kmin, dims = key_box(u8(base))
    assert (dims <= np.array(GRID_DIMS)).all(), dims
    pkey = kmin + np.array(GRID_DIMS) - 1 + [0, 0, dz_extra]
    o = ready(oracle_lib.Oracle(sc.cfg(), imu_mode_only=True), base)
    pw = patch_points(pkey, vs, 91 + dz_extra, N_PATCH, 0.01)
    o.map_update(pw, np.tile((1e-4 * np.eye(3)).reshape(1, 9), (N_PATCH, 1)))
    blob = bytes(o.map_export())
    kmin2, dims2 = key_box(u8(blob))
    cells = int(np.prod(dims2))
    assert (kmin2 == kmin).all() and tuple(kmin2 + dims2 - 1) == tuple(pkey), (kmin2, dims2, pkey)
    scans, xs, Ps = batch_of(sc, tp, seed=7007)
    centre = (pkey + 0.5) * vs
    xs[0] = offconfig.identity_state(pos=centre + [-2.0, 1.5, 1.6583], rotvec=(0.02, -0.03, 0.4))    # |offset| = 3.0 m
    on = offconfig.body_of(xs[0], patch_points(pkey, vs, 191 + dz_extra, N_ON_PATCH, 0.002), sc.P)
    scans[0]["x"][:N_ON_PATCH], scans[0]["y"][:N_ON_PATCH], scans[0]["z"][:N_ON_PATCH] = on[:, 0], on[:, 1], on[:, 2]
    o.set_state(xs[0], Ps[0])
    n_valid = int(o.residuals(scenes.xyz_of(scans[0])[:N_ON_PATCH])[3].sum())
    assert n_valid >= 250, n_valid
    o.close()
    _cache[key] = dict(sc=sc, base=base, blob=blob, pkey=pkey, cells=cells, scans=scans, xs=xs, Ps=Ps, n_valid=n_valid)
    return _cache[key]


def frozen_both(g, c):
    """The case's batch through lk_batch_replay_dev (as given) and lk_batch_replay_ragged_dev."""
    off, dt = synth.buckets_of(c["scans"][0])
    allpts = np.concatenate(c["scans"])
    d_pts = g.device_malloc(allpts.nbytes)
    g.h2d(d_pts, allpts)
    g.batch_order(0)
    g.batch_set_priors(np.array(c["xs"]), np.array(c["Ps"]))
    uni = grab(g, g.batch_replay_dev(d_pts, S, N_PTS, 0.0, off, dt))
    g.batch_set_priors(np.array(c["xs"]), np.array(c["Ps"]))
    rag = grab(g, g.batch_replay_ragged_dev(d_pts, g.ragged_tables(np.arange(S + 1) * N_PTS, [off] * S, [dt] * S, [0.0] * S)))
    g.batch_order(1)
    g.device_free(d_pts)
    return uni, rag


def overlay_errors(hip_lib, g, c, code, *words):
    """Both overlay entries refuse the case's batch with `code`, every one of `words` in the message."""
    off, dt = synth.buckets_of(c["scans"][0])
    calls = (lambda: g.batch_replay_overlay(c["scans"], 0.0, off, dt),
             lambda: g.batch_replay_overlay_ragged(c["scans"], [0.0] * S, c["xs"], c["Ps"]))
    for call in calls:
        g.batch_set_priors(np.array(c["xs"]), np.array(c["Ps"]))
        with pytest.raises(hip_lib.LegKiloError) as e:
            call()
        assert f"error {code}:" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def check_case_against_the_oracle(oracle_lib, c, got, where):
    o = ready(oracle_lib.Oracle(c["sc"].cfg(), imu_mode_only=True), c["blob"])
    want = oracle_frozen(o, c["scans"], [0.0] * S, c["xs"], c["Ps"])
    o.close()
    worst = check_abs(want, got, where)
    assert want[0][2] >= c["n_valid"] >= 250, (where, want[0][2], c["n_valid"])     # slot 0 counts the patch points (nothing else is in reach of its prior)
    assert min(w[2] for w in want[1:]) > 300
    return worst


def test_grid_just_under_the_cap(oracle_lib, hip_lib, monkeypatch):
    """A key box of 256 x 256 x 250 = 16 384 000 cells (2.36 GB of 144-byte records; the match pool grows to 1.25 x that): the patch's
    record is the LAST cell, 2.36 GB into the pool - beyond a signed and close to an unsigned 32-bit byte offset.  Frozen replay
    (uniform and ragged) bit-equal to the LEGKILO_GRID=0 handle and at parity with the oracle; slot 0 matches the patch; the overlay
    replay succeeds and passes overlay_replay_and_check for slot 0, so the grid is on and the per-cell bitmaps reach the last cell."""
    c = grid_limit_case(oracle_lib, 0)
    assert 0.95 * 2 ** 24 < c["cells"] <= 2 ** 24, c["cells"]
    sc = c["sc"]
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), c["blob"])
    g0 = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), c["blob"])
    uni, rag = frozen_both(g, c)
    uni0, rag0 = frozen_both(g0, c)
    same_bits(uni, uni0, "uniform: grid vs LEGKILO_GRID=0")
    same_bits(rag, rag0, "ragged: grid vs LEGKILO_GRID=0")
    same_bits(uni, rag, "uniform vs ragged")
    worst = check_case_against_the_oracle(oracle_lib, c, uni, "under the cap")
    print(f"grid of {c['cells']} cells: slot 0 n_effect {uni[0][2]} ({c['n_valid']} of {N_ON_PATCH} patch points valid), max |dx| {worst:.2e}")
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    o.init_process_cov_q()
    tcs.overlay_replay_and_check(o, g, "under the cap", u8(c["blob"]), c["scans"][:1], c["xs"][:1], c["Ps"][:1], (16384, 32768, 16384), least_effect=249)
    tcs.close(g0, g, o)


def test_grid_over_the_cap(oracle_lib, hip_lib, monkeypatch):
    """The same patch 8 voxels further out in z: 256 x 256 x 258 cells > kGridMaxCells, so frozen_map() stays on the hash table BY ITSELF
    (not forced by LEGKILO_GRID=0).  Frozen replay at parity with the oracle and bit-equal to the forced-hash handle; both overlay
    entries return LK_ERR_STATE naming the frozen-map grid; the handle stays usable - the next frozen replay repeats the first."""
    c = grid_limit_case(oracle_lib, 8)
    assert 2 ** 24 < c["cells"] <= 1.1 * 2 ** 24, c["cells"]
    sc = c["sc"]
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), c["blob"])
    g0 = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), c["blob"])
    uni, rag = frozen_both(g, c)
    uni0, rag0 = frozen_both(g0, c)
    same_bits(uni, uni0, "uniform: fallback vs LEGKILO_GRID=0")
    same_bits(rag, rag0, "ragged: fallback vs LEGKILO_GRID=0")
    worst = check_case_against_the_oracle(oracle_lib, c, uni, "over the cap")
    print(f"key box of {c['cells']} cells: hash fallback, slot 0 n_effect {uni[0][2]}, max |dx| {worst:.2e}")
    overlay_errors(hip_lib, g, c, LK_ERR_STATE, "frozen-map grid")
    uni2, rag2 = frozen_both(g, c)
    same_bits(uni2, uni, "uniform after the refusals")
    same_bits(rag2, rag, "ragged after the refusals")
    tcs.close(g0, g)


@pytest.mark.parametrize("poison", [False, True])
def test_grid_there_and_back_on_one_handle(oracle_lib, hip_lib, monkeypatch, poison):
    """One handle through the grid's states: the base map (small grid) -> lk_map_update of the first patch (the grid grows to 16.4 M cells,
    the match pool is replaced) -> the second patch (fallback to the hash table, overlay refused) -> lk_map_clear_outside with the base
    box (both patches leave; back on a small grid).  Every replay equals that of a fresh handle holding the same map, bit for bit; at
    the end the overlay replay does too.  Once more with LEGKILO_POISON_POOLS=1 (fresh pools hold 0x5a bytes)."""
    if poison:
        monkeypatch.setenv("LEGKILO_POISON_POOLS", "1")
    ca, cb = grid_limit_case(oracle_lib, 0), grid_limit_case(oracle_lib, 8)
    sc, base = ca["sc"], ca["base"]
    vs = float(sc.P["voxel_size"])
    var = np.tile((1e-4 * np.eye(3)).reshape(1, 9), (N_PATCH, 1))
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), base)
    fresh = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), base)
    first = frozen_both(g, ca)
    same_bits(first[0], frozen_both(fresh, ca)[0], "base map")
    # ---- the first patch: the grid grows to GRID_DIMS, the match pool is replaced
    g.map_update(patch_points(ca["pkey"], vs, 91, N_PATCH, 0.01), var)
    blob_a = g.map_export()
    scenes.compare_maps(u8(ca["blob"]), blob_a)      # the oracle built ca["blob"] by the same insert into the same base map
    fresh_a = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), blob_a)
    ua, ra = frozen_both(g, ca)
    fa = frozen_both(fresh_a, ca)
    same_bits(ua, fa[0], "after the first patch: uniform")
    same_bits(ra, fa[1], "after the first patch: ragged")
    assert ua[0][2] >= 250 and first[0][0][2] == 0, (ua[0][2], first[0][0][2])      # slot 0 matches the patch, and nothing was there before
    # (no state comparison with the oracle here: this handle fitted the patch's plane itself, 170 m from the origin, where two correct
    # fits differ by ~0.1 B = 2e-9 in the normal and by an ulp of the float d, 1.5e-5 m, and slot 0 sees that one plane only - measured
    # 1.7e-8 on a rotation entry.  The open-loop comparison on the oracle's own blob is test_grid_just_under_the_cap.)
    fresh_a.close()
    # ---- the second patch: over the cap, back to the hash table
    g.map_update(patch_points(cb["pkey"], vs, 91 + 8, N_PATCH, 0.01), var)
    fresh_b = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), g.map_export())
    ub, rb = frozen_both(g, ca)
    fb = frozen_both(fresh_b, ca)
    same_bits(ub, fb[0], "after the second patch (hash table): uniform")
    same_bits(rb, fb[1], "after the second patch (hash table): ragged")
    assert ub[0][2] >= 250, ub[0][2]
    fresh_b.close()
    overlay_errors(hip_lib, g, ca, LK_ERR_STATE, "frozen-map grid")
    kmin, dims = key_box(u8(base))
    kmax = kmin + dims - 1
    assert g.map_clear_outside(int(kmax[0]), int(kmin[0]), int(kmax[1]), int(kmin[1]), int(kmax[2]), int(kmin[2])) == 2
    scenes.maps_identical(g.map_export(), u8(base))
    back = frozen_both(g, ca)
    same_bits(back[0], first[0], "back on the base map: uniform")
    same_bits(back[1], first[1], "back on the base map: ragged")
    off, dt = synth.buckets_of(ca["scans"][0])
    res = []
    for h in (g, fresh):
        h.overlay_reserve(16384, 32768, 16384)
        h.batch_set_priors(np.array(ca["xs"]), np.array(ca["Ps"]))
        res.append((grab(h, h.batch_replay_overlay(ca["scans"], 0.0, off, dt)), [bytes(h.overlay_export(s)) for s in range(S)]))
    same_bits(res[0][0], res[1][0], "overlay replay back on the base map")
    for s in range(S):
        scenes.maps_identical(u8(res[0][1][s]), u8(res[1][1][s]))
    tcs.close(fresh, g)


def test_packed_key_range_of_the_overlay(oracle_lib, hip_lib, monkeypatch):
    """`edge`: x keys around 1.2 M, past the +-2^20 of the overlay's packed root keys.  The frozen replay does not pack keys: grid = hash,
    bit for bit (no oracle comparison: the reference itself is good to 1e-4 only at 600 km).  Both overlay entries return
    LK_ERR_INVALID, the message naming the key range and the slot; the priors are intact afterwards, and a following frozen replay
    repeats the earlier one bit for bit."""
    sc = placement.placed_scene("edge", **CAPS)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    x0 = scenes.init_filter(o, sc, T0)
    scenes.first_frame(o, sc, T0, x0)
    blob = bytes(o.map_export())
    o.close()
    kmin, dims = key_box(u8(blob))
    assert kmin[0] > 2 ** 20, kmin
    scans, xs, Ps = batch_of(sc, T0)
    c = dict(scans=scans, xs=xs, Ps=Ps)
    g = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S)), blob)
    g0 = ready(tcs.grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch), blob)
    uni, rag = frozen_both(g, c)
    uni0, rag0 = frozen_both(g0, c)
    same_bits(uni, uni0, "uniform: grid vs LEGKILO_GRID=0")
    same_bits(rag, rag0, "ragged: grid vs LEGKILO_GRID=0")
    assert min(r[2] for r in uni) > 300, [r[2] for r in uni]
    off, dt = synth.buckets_of(scans[0])
    for call in (lambda: g.batch_replay_overlay(scans, 0.0, off, dt), lambda: g.batch_replay_overlay_ragged(scans, [0.0] * S)):
        g.batch_set_priors(np.array(xs), np.array(Ps))
        with pytest.raises(hip_lib.LegKiloError) as e:
            call()
        msg = str(e.value)
        assert f"error {LK_ERR_INVALID}:" in msg and "2^20" in msg and "slot " in msg, msg
        X, P = g.batch_get_states(0, S)
        assert np.array_equal(X, np.array(xs)) and np.array_equal(P, np.array(Ps)), "a refused overlay replay must leave the priors in the slots"
    uni2, rag2 = frozen_both(g, c)
    same_bits(uni2, uni, "uniform after the refusals")
    same_bits(rag2, rag, "ragged after the refusals")
    tcs.close(g0, g)


# ============================================================================= 3e. closed loop at negz, full tolerances
# `negz` conditions like the origin (|p| < 30 m), so the suite's closed-loop bars hold there: the existing drivers and assertions, on the moved scene.
@pytest.mark.parametrize("use_kin", [False, True])
def test_closed_loop_sequence_at_negz(oracle_lib, hip_lib, use_kin):
    """test_sequence_scan_resident_and_launches (scan-resident kernel = per-bucket launches bit for bit, both against the oracle at its
    tolerances), 4 scans, IMU-only and leg fusion, with every z key negative."""
    sc = placement.placed_scene("negz", None, use_kin, **CAPS)
    tcs.sequence_scan_resident_and_launches(oracle_lib, hip_lib, "negz", use_kin, scene=sc, n_scans=4)


def test_closed_loop_grid_resident_at_negz(oracle_lib, hip_lib):
    """test_scan_grid_kernel_and_launches (grid-resident kernel = per-bucket launches, both against the oracle), 5 buckets."""
    tcs.scan_grid_kernel_and_launches(oracle_lib, hip_lib, "negz", 5, scene=placement.placed_scene("negz", **CAPS))


def test_closed_loop_overlay_scattered_at_negz(oracle_lib, hip_lib):
    """test_batch_replay_overlay_scattered: lk_batch_replay_overlay_dev against the oracle's KILO::process on a private map, slot by slot."""
    tcs.batch_replay_overlay_scattered(oracle_lib, hip_lib, "negz", scene=placement.placed_scene("negz", **CAPS))


def test_closed_loop_overlay_ragged_at_negz(oracle_lib, hip_lib, monkeypatch):
    """test_batch_replay_overlay_ragged_scan_resident_imu: lk_batch_replay_overlay_ragged_dev scan-resident and with LEGKILO_RAG_RESIDENT=0."""
    tcs.batch_replay_overlay_ragged_scan_resident_imu(oracle_lib, hip_lib, monkeypatch, "negz", scene=placement.placed_scene("negz", **CAPS))


def test_closed_loop_run_with_map_sliding_at_negz(hip_lib):
    """test_run_with_map_sliding: lk_run_scans_dev with map sliding against the lk_process_scan + lk_map_slide loop, bit for bit."""
    import test_live_run as tlr

    tlr.run_with_map_sliding(hip_lib, placed("negz"))


def placed(place):
    """One scene object per placement (test_live_run caches its scans by scene)."""
    if ("scene", place) not in _cache:
        _cache[("scene", place)] = placement.placed_scene(place, **CAPS)
    return _cache[("scene", place)]


# ============================================================================= 3f. kernel variants agree at neg and far
@pytest.mark.parametrize("place", ["neg", "far"])
def test_kernel_variants_agree(oracle_lib, hip_lib, monkeypatch, place):
    """Device against device, no tolerance - identities that hold by design at any placement, 3 scans with insert:
    scan-resident kernel = per-bucket launches (config-1 scans) and grid-resident kernel = per-bucket launches = the default choice
    (2 000-point buckets): states and covariances bit for bit, maps by maps_identical; lk_run_scans_dev = the lk_process_scan loop;
    lk_batch_replay_overlay_ragged_dev scan-resident = launch by launch.  Against the oracle only the first scan's match count: beyond it
    the reference's own refits set the tolerance (tests/test_placement_pin.py)."""
    import test_live_run as tlr

    sc = placed(place)
    t0 = 2.0
    # ---- config-1 scans: scan-resident, per-bucket launches, the one-call run
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    g, g_pb, g_run = (hip_lib.LegKiloHip(sc.cfg()) for _ in range(3))
    g_pb.stream_resident(False)
    for obj in (o, g, g_pb, g_run):
        tlr._start(obj, sc, t0)
    scans = [scenes.vlp_scan_input(sc, t0 + 0.1 * k, k) for k in range(3)]
    tbs = [t0 + 0.1 * k for k in range(3)]
    imus = [synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k) for k, tb in enumerate(tbs)]
    po, _ = o.process_scan(scans[0], tbs[0], imus=imus[0])
    ref_poses, ref_worlds, _ = tlr._loop(g, scans, tbs, 1, imus)
    pb_poses, pb_worlds, _ = tlr._loop(g_pb, scans, tbs, 1, imus)
    assert (po.n_buckets, po.n_updates, int(po.n_effect)) == (ref_poses[0].n_buckets, ref_poses[0].n_updates, int(ref_poses[0].n_effect)), (po.n_effect, ref_poses[0].n_effect)
    assert po.n_effect > 300
    run_poses, run_worlds, _ = g_run.run_scans(scans, tbs, world=True, imus=imus)
    for s in range(3):
        tlr._same_pose(pb_poses[s], ref_poses[s], (place, "per-bucket", s))
        tlr._same_pose(run_poses[s], ref_poses[s], (place, "run", s))
        assert np.array_equal(pb_worlds[s], ref_worlds[s]) and np.array_equal(run_worlds[s], ref_worlds[s]), (place, s)
    assert tlr._same_handle_state(g_pb, g) > 100 and tlr._same_handle_state(g_run, g) > 100
    assert g.stream_resident_stats()[0] == 3 and g_pb.stream_resident_stats()[0] == 0
    blob = g.map_export()
    tcs.close(g_pb, g_run, o)
    # ---- recorded-run replay with insert on that map: scan-resident = launch by launch
    rng = np.random.default_rng(717171)
    S4 = 4
    rtb = [t0 + 0.4 + 0.23 * s for s in range(S4)]
    rscans = [scenes.vlp_scan_input(sc, rtb[s], 180 + s) for s in range(S4)]
    rxs = [synth.initial_state(sc.traj, rtb[s], sc.P, rng, 0.02, 0.5) for s in range(S4)]
    rPs = [1e-4 * np.eye(30)] * S4
    rimus = [synth.imu_stream(sc.traj, rtb[s], rtb[s] + 0.1, seed=9500 + s) for s in range(S4)]
    gr = ready(hip_lib.LegKiloHip(sc.cfg(n_slots=S4)), bytes(blob))
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    res = grab(gr, gr.batch_replay_overlay_ragged(rscans, rtb, rxs, rPs, imus=rimus))
    assert gr.overlay_resident_rounds() >= 1, "the scan-resident form did not run"
    exports = [bytes(gr.overlay_export(s)) for s in range(S4)]
    monkeypatch.setenv("LEGKILO_RAG_RESIDENT", "0")
    res0 = grab(gr, gr.batch_replay_overlay_ragged(rscans, rtb, rxs, rPs, imus=rimus))
    assert gr.overlay_resident_rounds() == 0
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT")
    same_bits(res, res0, (place, "overlay ragged: scan-resident vs launch by launch"))
    assert min(r[2] for r in res) > 300, [r[2] for r in res]
    for s in range(S4):
        assert scenes.maps_identical(gr.overlay_export(s), u8(exports[s])), (place, s)
    tcs.close(gr, g)
    # ---- 2 000-point buckets: grid-resident kernel, per-bucket launches, the default choice
    hs = [hip_lib.LegKiloHip(sc.cfg()) for _ in range(3)]
    hs[0].stream_grid(2)
    hs[1].stream_grid(0)
    hs[1].stream_resident(False)
    for h in hs:
        x0 = scenes.init_filter(h, sc, t0)
        scenes.first_frame(h, sc, t0, x0, dense=20000)
    for k in range(3):
        tb = t0 + 0.1 * k
        pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=N_PTS, n_buckets=NB, seed_scan=9300 + k, seed_noise=9400 + k)
        out = [h.process_scan(pts, tb, want_world=True) for h in hs]
        for (p, w), h in zip(out[1:], hs[1:]):
            tlr._same_pose(p, out[0][0], (place, "dense", k))
            assert np.array_equal(w, out[0][1]), (place, k)
        assert out[0][0].n_effect > 1000
    assert hs[0].stream_resident_stats()[0] == 3 and hs[1].stream_resident_stats()[0] == 0, (hs[0].stream_resident_stats(), hs[1].stream_resident_stats())
    for h in hs[1:]:
        assert tlr._same_handle_state(h, hs[0]) > 100
    tcs.close(*hs)
