"""-m gpu parity AWAY from the shipped configuration: the HIP path against the CPU oracle, per entry-point family, at every
configuration of tests/offconfig.py - a tilted 6-decimal extrinsic rotation (the generic kernel instantiations with ext_R != I),
voxel size 0.4 (the divide branch of key_trunc, float vs double key divisor), max_layer 0 / 3 / 4 with per-layer thresholds and an
early freeze, other gate constants.  tests/test_reference_pin.py pins the oracle against the reference's own build at the same
configurations, which is what makes it a checker here.  Call sequences and tolerances are those of the tests of
tests/test_gpu_parity.py named in each docstring; decisions (valid masks, found / success / layer, n_effect, tree shape, counters,
state bits) are exact.

The divide branch of key_trunc is covered by being executed at 0.4 and by the closed-loop counts only: a wrong divisor there moves
a key for points within ~1e-8 of a voxel face, which random scenes do not contain.  The float divisor of the INSERT key is pinned
by the face lattice of test_face_lattice_root_keys.
"""
import numpy as np
import pytest

import offconfig
import scenes
from legkilo_amd import synth

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
N_SITES, PER_SHEET = 10, 8000


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


def make_pair(name, oracle_lib, hip_lib, use_kin=False, scene=None, **over):
    """scene: a ready scene (tests/placement.py) instead of the one offconfig builds from the configuration's name."""
    sc = scene or offconfig.scene(name, use_kin, **CAPS)
    return sc, oracle_lib.Oracle(sc.cfg(**over), imu_mode_only=not use_kin), hip_lib.LegKiloHip(sc.cfg(**over))


def close(*objs):
    for obj in objs:
        obj.close()


def expected_depth(P):
    """Levels a crafted scene can reach: a cell of side a holds no point set whose smallest eigenvalue exceeds a^2 / 4, so with
    min_eigen_value 0.01 nothing below layer 1 (a = 0.25 m at voxel size 0.5) is ever cut: depth 3 at most.  With 5e-5 (deep4 /
    deep3) every layer down to max_layer is."""
    if P["min_eigen_value"] >= 0.01:
        return min(P["max_layer"], 2) + 1
    return P["max_layer"] + 1


def assert_deep(blob, P):
    cm = scenes.canon_map(blob)
    d = expected_depth(P)
    assert offconfig.depth(cm) == d, (offconfig.depth(cm), d)
    nodes, planes = offconfig.layer_counts(cm)
    assert (nodes[:d] > 0).all() and (nodes[d:] == 0).all(), nodes
    return nodes, planes


_cache = {}


def mature_oracle(name, oracle_lib, n_scans=10):
    """A live oracle after a first frame + n_scans config-1 scans at configuration `name` (z = 0 forced on every 37th raw point)."""
    sc = offconfig.scene(name, **CAPS)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    t0 = 1.0
    x0 = scenes.init_filter(o, sc, t0)
    scenes.first_frame(o, sc, t0, x0)
    scenes.replay_vlp(o, sc, t0, n_scans, scan_input=offconfig.ZeroZ())
    return o


def mature_blob(name, oracle_lib, n_scans=10):
    """Map, state, covariance and times of mature_oracle, cached per module run."""
    key = ("mature", name, n_scans)
    if key not in _cache:
        o = mature_oracle(name, oracle_lib, n_scans)
        xs, Ps = o.get_state()
        _cache[key] = (bytes(o.map_export()), xs, Ps, o.get_times())
        o.close()
    return _cache[key]


def matured(name, oracle_lib, hip_lib, live=False, **over):
    """(scene, oracle, handle) both holding the matured map, state, covariance and times.  live: the oracle holds the map it grew
    itself - needed wherever maps are compared after further inserts, because the blob does not carry the stored points of cut
    inner nodes (never read again) and an oracle that imported it would count them as 0."""
    blob, xs, Ps, (tp, tu) = mature_blob(name, oracle_lib)
    sc, o, g = make_pair(name, oracle_lib, hip_lib, **over)
    if live:
        o.close()
        o = mature_oracle(name, oracle_lib)
        assert np.array_equal(o.get_state()[0], xs) and bytes(o.map_export()) == blob
    for obj in ((g,) if live else (o, g)):
        obj.map_import(np.frombuffer(blob, dtype=np.uint8))
    for obj in (o, g):
        obj.set_state(xs, Ps)
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
        obj.set_times(tp, tu)
    return sc, o, g, xs, Ps, tp


def sites():
    if "sites" not in _cache:
        _cache["sites"] = offconfig.CornerSites(seed=71, n_sites=N_SITES, per_sheet=PER_SHEET)
    return _cache["sites"]


def site_oracle(name, oracle_lib):
    """A live oracle holding the corner-site map (N_SITES sites) + the uniform box, built by its UpdateVoxelMap at configuration `name`."""
    o = oracle_lib.Oracle(offconfig.scene(name, **CAPS).cfg(), imu_mode_only=True)
    p, var = sites().points()
    o.map_update(p, var)
    pb, vb = offconfig.uniform_box(seed=61, n=20000, offset=(0.0, 3.0, 0.0))
    o.map_update(pb, vb)
    return o


def site_blob(name, oracle_lib):
    """The map of site_oracle as a blob, cached per module run."""
    key = ("site", name)
    if key not in _cache:
        P = offconfig.params(name)
        o = site_oracle(name, oracle_lib)
        blob = bytes(o.map_export())
        nodes, planes = assert_deep(blob, P)
        assert (planes[1: P["max_layer"] + 1] > 0).all(), planes
        print(f"{name} corner-site map: nodes per layer {nodes}, planes per layer {planes}")
        _cache[key] = blob
        o.close()
    return np.frombuffer(_cache[key], dtype=np.uint8)


def site_state(k=0):
    """A body pose near the sites: small rotation, so that body z = 0 stays (to millimetres) on the vertical sheets."""
    return offconfig.identity_state(pos=(0.013 + 0.002 * k, -0.021, 0.55 + 0.001 * k), rotvec=(0.004, -0.003, 0.005 + 0.001 * k))


def site_queries(P, x, seed, n_per_sheet=700):
    """`fresh` site points in the body frame of x, z = 0 forced on every 37th one."""
    pw, _ = sites().fresh(seed, n_per_sheet)
    xb = offconfig.body_of(x, pw, P)
    xb[::37, 2] = 0.0
    return xb


def check_mask_and_rows(o, tag, xb, ro, rg, max_flips=1):
    """The rule of test_config2_full_size_residuals: masks equal except for at most one NAMED flip per 100 000 points whose gate
    margin is at rounding level (< 1e-9); rows 1e-9 on the points both hold valid."""
    (ho, zo, Ro, vo), (hg, zg, Rg, vg) = ro, rg
    flips = np.flatnonzero(vo != vg)
    for i in flips:
        _, marg = o.residual_margins(xb[i])
        print(f"{tag} flip: point {int(i)} oracle valid {int(vo[i])} hip valid {int(vg[i])} margins range/sigma/key {marg}")
        assert min(marg[0], marg[1]) < 1e-9 or marg[2] < 1e-9, (tag, int(i), marg)
    assert len(flips) <= max_flips, (tag, flips)
    scenes.rows_close(hg, zg, Rg, ho, zo, Ro, (vo & vg).astype(np.uint8), rtol=1e-9)
    return len(flips)


# ============================================================================= 1. map build and insert
@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_map_build_dense_first_frame(oracle_lib, hip_lib, name):
    """test_map_build_parity: lk_map_build on a dense first frame - point_geom through a tilted ext_R, roots keyed at 0.4."""
    sc, o, g = make_pair(name, oracle_lib, hip_lib)
    t0 = 1.0
    for obj in (o, g):
        x0 = scenes.init_filter(obj, sc, t0)
        scenes.first_frame(obj, sc, t0, x0, dense=60000)
    stats = scenes.compare_maps(o.map_export(), g.map_export())
    print(name, stats)
    assert stats["roots"] > 1000 and stats["planes"] > 500     # (at 0.4 m no voxel of this frame is cut: nodes == roots)
    close(g, o)


@pytest.mark.parametrize("name", ["deep4", "deep3", "desc4", "layers3", "layer0"])
def test_map_crafted_scenes_update_and_build(oracle_lib, hip_lib, name):
    """test_map_build_clutter / test_map_update_surface at tree depths 1, 4 and 5: the uniform box and the corner sites fed through
    lk_map_update in chunks of 1, 1, 5, 17, 200, 1 000, 5 000, rest (compare_maps after every chunk), then corner_clutter; and the
    same points, expressed in the body frame of a rotated state, through lk_map_build, then corner_clutter through lk_map_update."""
    big = dict(max_scan_points=1 << 19)     # the rest of the sites (234 000 points) goes in as ONE call
    sc, o, g = make_pair(name, oracle_lib, hip_lib, **big)
    P = sc.P
    rng = np.random.default_rng(81)
    box, box_var = offconfig.uniform_box(seed=61, n=40000)
    sp, sp_var = sites().points()
    clutter = scenes.corner_clutter(rng, 50, 40)
    cvar = np.tile((np.eye(3) * 4e-4).reshape(1, 9), (len(clutter), 1))
    for pts, var in ((box, box_var), (sp, sp_var), (clutter, cvar)):
        for a, b in offconfig.chunks_of(len(pts)):
            for obj in (o, g):
                obj.map_update(pts[a:b], var[a:b])
            scenes.compare_maps(o.map_export(), g.map_export())
    nodes, planes = assert_deep(g.map_export(), P)
    print(f"{name} lk_map_update: nodes per layer {nodes}, planes per layer {planes}")
    close(g, o)
    # ---- BuildVoxelMap on the same world, seen from a rotated body
    sc, o, g = make_pair(name, oracle_lib, hip_lib, **big)
    x = offconfig.identity_state(pos=(1.0, -2.0, 0.4), rotvec=(0.1, -0.2, 0.7))
    pw = np.concatenate([box + [0.0, 3.0, 0.0], sp, clutter + [0.0, 6.0, 0.0]])
    rng.shuffle(pw)
    xb = offconfig.body_of(x, pw, P)
    xw = scenes.world_of(x, xb, P)
    for obj in (o, g):
        obj.set_state(x, 1e-6 * np.eye(30))
        obj.map_build(xw, xb)
    scenes.compare_maps(o.map_export(), g.map_export())
    nodes, planes = assert_deep(g.map_export(), P)
    print(f"{name} lk_map_build: nodes per layer {nodes}, planes per layer {planes}")
    extra = scenes.corner_clutter(rng, 40, 30) + [0.0, 6.0, 0.0]
    A = rng.normal(size=(len(extra), 3, 3)) * 0.01
    evar = (A @ A.transpose(0, 2, 1) + 1e-5 * np.eye(3)).reshape(-1, 9)
    for obj in (o, g):
        obj.map_update(extra, evar)
    scenes.compare_maps(o.map_export(), g.map_export())
    close(g, o)


def test_face_lattice_root_keys(oracle_lib, hip_lib):
    """Points exactly on the faces of the 0.4 m grid through lk_map_update at the identity state.  The insert key divides by the FLOAT
    voxel size (voxel_map.cc:337; key_floor of lk_device.h), so the root keys are not floor(p / 0.4): the device's exported root-key
    set equals the oracle's (pinned against the reference on the same lattice), and the double divisor's set differs from both."""
    sc, o, g = make_pair("vs04", oracle_lib, hip_lib)
    p, var = offconfig.face_lattice(sc.P["voxel_size"])
    for obj in (o, g):
        obj.set_state(offconfig.identity_state(), 1e-6 * np.eye(30))
        obj.map_update(p, var)
    ko, kg = set(scenes.canon_map(o.map_export())), set(scenes.canon_map(g.map_export()))
    naive = offconfig.naive_keys(p, sc.P["voxel_size"])
    print(f"face lattice: {len(ko)} root voxels, {len(ko ^ naive)} entries differ from floor(p / 0.4), device differs from the oracle in {len(ko ^ kg)}")
    assert len(ko ^ naive) >= 10, "the lattice no longer tells the float divisor from the double one"
    assert kg == ko, sorted(kg ^ ko)[:10]
    scenes.compare_maps(o.map_export(), g.map_export())
    close(g, o)


# ============================================================================= 2. residual rows and the matcher
@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_residuals_and_batch_rows(oracle_lib, hip_lib, name):
    """test_residuals_on_imported_map + the reduced shape of test_config2_batch_rows_resident (4 slots x 20 000 points, each under its
    own perturbed state) on an oracle-matured map: lk_residuals and lk_batch_residuals_dev against the oracle (masks by the flip rule,
    rows 1e-9), the batch entry equal to the host entry bit for bit.  z = 0 forced on every 37th query point."""
    S, n_pts = 4, 20000
    sc, o, g, xs0, Ps0, tp = matured(name, oracle_lib, hip_lib, n_slots=S)
    rng = np.random.default_rng(2202)
    tbs = [tp + 0.3 + 0.21 * s for s in range(S)]
    scans = [synth.dense_scan(sc.world, scenes.Frozen(sc.traj, tbs[s]), tbs[s], sc.P, n=n_pts, n_buckets=1, seed_scan=2302 + s) for s in range(S)]
    for s_ in scans:
        s_["z"][::37] = 0.0
    xs = np.stack([synth.initial_state(sc.traj, tbs[s], sc.P, rng, 0.02, 0.5) for s in range(S)])
    Ps = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (S, 1))
    allpts = np.concatenate(scans)
    N = S * n_pts
    d_pts, d_rows, d_v = g.device_malloc(allpts.nbytes), g.device_malloc(N * 64), g.device_malloc(N)
    g.h2d(d_pts, allpts)
    g.batch_set_priors(xs, Ps)
    g.batch_residuals_dev(d_pts, S, n_pts, d_rows, d_v)
    g.synchronize()
    rows8, v = np.zeros((N, 8)), np.zeros(N, dtype=np.uint8)
    g.d2h(rows8, d_rows)
    g.d2h(v, d_v)
    for d in (d_pts, d_rows, d_v):
        g.device_free(d)
    h6, z, R = np.ascontiguousarray(rows8[:, :6]), np.ascontiguousarray(rows8[:, 6]), np.ascontiguousarray(rows8[:, 7])
    n_flips = n_zero_valid = n_zero = 0
    for s in range(S):
        a, b = s * n_pts, (s + 1) * n_pts
        xb = scenes.xyz_of(scans[s])
        o.set_state(xs[s], Ps[s].reshape(30, 30))
        ro = o.residuals(xb)
        assert ro[3].sum() > 2000, ro[3].sum()
        n_zero += int((xb[:, 2] == 0).sum())
        n_zero_valid += int(ro[3][xb[:, 2] == 0].sum())
        n_flips += check_mask_and_rows(o, f"{name} slot {s}", xb, ro, (h6[a:b], z[a:b], R[a:b], v[a:b]))
        unm = v[a:b] == 0
        assert not h6[a:b][unm].any() and not z[a:b][unm].any() and not R[a:b][unm].any()
        g.set_state(xs[s], Ps[s].reshape(30, 30), slot=0)    # the host entry: the same bits
        hh, zh, Rh, vh = g.residuals(xb)
        assert np.array_equal(vh, v[a:b]) and np.array_equal(hh, h6[a:b]) and np.array_equal(zh, z[a:b]) and np.array_equal(Rh, R[a:b]), s
    print(f"{name}: {n_zero} query points with z == 0, {n_zero_valid} of them valid, {n_flips} flips")
    assert n_flips <= 1 and n_zero >= 200 and n_zero_valid >= 50, (n_flips, n_zero, n_zero_valid)
    close(g, o)


def match_points_against_oracle(o, g, oracle_lib, keys, P, V):
    """lk_match_points == the oracle's build_single_residual, query by query (test_build_single_residual_per_point) -> successes per layer."""
    mg = g.match_points(keys, P, V)
    per_layer, n_found = {}, 0
    for i in range(len(keys)):
        mo = o.match_voxel(keys[i], P[i], V[i].reshape(9))
        assert (mo["found"], mo["success"]) == (bool(mg["found"][i]), bool(mg["success"][i])), (i, keys[i], mo, {k: v[i] for k, v in mg.items()})
        n_found += mo["found"]
        if mo["success"]:
            per_layer[mo["layer"]] = per_layer.get(mo["layer"], 0) + 1
            assert mo["layer"] == mg["layer"][i], (i, mo["layer"], mg["layer"][i])
            assert np.array_equal(mo["normal"], mg["normal"][i]) and np.array_equal(mo["center"], mg["center"][i])
            assert mo["d"] == mg["d"][i]
            assert np.isclose(mo["dis_to_plane"], mg["dis_to_plane"][i], rtol=1e-6, atol=1e-9)
            assert np.isclose(mo["prob"], mg["prob"][i], rtol=1e-9), (mo["prob"], mg["prob"][i])
        else:
            assert mg["layer"][i] == -1 and mg["prob"][i] == 0.0
    return per_layer, n_found


@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_match_points_per_point(oracle_lib, hip_lib, name):
    """test_build_single_residual_per_point: caller-held world points and covariances on their home voxel (keyed with the DOUBLE voxel
    size, as the residual side does) and three neighbouring keys, on the matured map + clutter that cuts voxels."""
    sc, o, g, xs, Ps, tp = matured(name, oracle_lib, hip_lib)
    rng = np.random.default_rng(41)
    clutter = scenes.corner_clutter(rng, n_cells=40, per_cell=70)
    o.map_update(clutter, np.tile((np.eye(3) * 4e-4).reshape(1, 9), (len(clutter), 1)))
    blob = o.map_export()
    g.map_import(blob)
    ts = tp + 0.5
    pts = synth.dense_scan(sc.world, scenes.Frozen(sc.traj, ts), ts, sc.P, n=2000, n_buckets=1)
    pw = scenes.world_of(synth.initial_state(sc.traj, ts, sc.P), scenes.xyz_of(pts), sc.P).astype(np.float64) + rng.normal(0, 0.03, (len(pts), 3))
    pw = np.concatenate([pw, clutter[:800] + rng.normal(0, 0.01, (800, 3)), rng.uniform(-30, 30, (200, 3))])
    vs = float(sc.P["voxel_size"])
    keys, Pq, V = [], [], []
    for i, p in enumerate(pw):
        k0 = oracle_lib.key_floor(p, vs)
        A = rng.normal(size=(3, 3))
        var = (A @ A.T) * (1e-5 if i % 3 else 4e-3) + np.eye(3) * 1e-6
        for dk in ((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1)):
            keys.append([a + b for a, b in zip(k0, dk)]), Pq.append(p), V.append(var)
    keys, Pq, V = np.array(keys, dtype=np.int32), np.array(Pq), np.array(V)
    per_layer, n_found = match_points_against_oracle(o, g, oracle_lib, keys, Pq, V)
    n_ok = sum(per_layer.values())
    print(f"{name}: found {n_found} of {len(keys)}, successes per layer {per_layer}")
    assert n_found > 2000 and n_ok > 1000 and n_ok - per_layer.get(0, 0) > 20, (n_found, per_layer)
    assert n_found < len(keys)
    scenes.compare_maps(blob, g.map_export())
    close(g, o)


@pytest.mark.parametrize("name", ["deep4", "deep3"])
def test_residuals_and_matcher_on_the_corner_sites(oracle_lib, hip_lib, name):
    """Layers 3 and 4 of the tree walk: lk_match_points, lk_residuals and lk_batch_residuals_dev on the corner-site map with `fresh`
    site points as queries - at least 100 matches on EACH layer 1 .. max_layer (counted on the oracle's side), at least 200 query
    points with z == 0 exactly, at least 50 of those valid."""
    S = 4
    sc, o, g = make_pair(name, oracle_lib, hip_lib, n_slots=S)
    P, L = sc.P, sc.P["max_layer"]
    blob = site_blob(name, oracle_lib)
    for obj in (o, g):
        obj.map_import(blob)
        obj.init_process_cov_q()
    # ---- the matcher, world points
    pw, var = sites().fresh(1, n_per_sheet=120)
    keys = np.array([oracle_lib.key_floor(p, float(P["voxel_size"])) for p in pw], dtype=np.int32)
    per_layer, _ = match_points_against_oracle(o, g, oracle_lib, keys, pw, var.reshape(-1, 3, 3))
    print(f"{name}: lk_match_points successes per layer {per_layer}")
    assert all(per_layer.get(l, 0) >= 100 for l in range(1, L + 1)), per_layer
    # ---- residual rows, body points under S states
    xs = np.stack([site_state(s) for s in range(S)])
    Ps = np.tile((1e-6 * np.eye(30)).reshape(1, 900), (S, 1))
    xbs = [site_queries(P, xs[s], 10 + s, n_per_sheet=420) for s in range(S)]
    n_pts = len(xbs[0])
    allpts = np.concatenate([offconfig.deal_buckets(xb, 1) for xb in xbs])
    N = S * n_pts
    d_pts, d_rows, d_v = g.device_malloc(allpts.nbytes), g.device_malloc(N * 64), g.device_malloc(N)
    g.h2d(d_pts, allpts)
    g.batch_set_priors(xs, Ps)
    g.batch_residuals_dev(d_pts, S, n_pts, d_rows, d_v)
    g.synchronize()
    rows8, v = np.zeros((N, 8)), np.zeros(N, dtype=np.uint8)
    g.d2h(rows8, d_rows)
    g.d2h(v, d_v)
    for d in (d_pts, d_rows, d_v):
        g.device_free(d)
    h6, z, R = np.ascontiguousarray(rows8[:, :6]), np.ascontiguousarray(rows8[:, 6]), np.ascontiguousarray(rows8[:, 7])
    n_flips = n_zero = n_zero_valid = n_valid = 0
    for s in range(S):
        a, b = s * n_pts, (s + 1) * n_pts
        o.set_state(xs[s], Ps[s].reshape(30, 30))
        ro = o.residuals(xbs[s])
        n_valid += int(ro[3].sum())
        n_zero += int((xbs[s][:, 2] == 0).sum())
        n_zero_valid += int(ro[3][xbs[s][:, 2] == 0].sum())
        n_flips += check_mask_and_rows(o, f"{name} slot {s}", xbs[s], ro, (h6[a:b], z[a:b], R[a:b], v[a:b]))
        g.set_state(xs[s], Ps[s].reshape(30, 30), slot=0)
        hh, zh, Rh, vh = g.residuals(xbs[s])
        assert np.array_equal(vh, v[a:b]) and np.array_equal(hh, h6[a:b]) and np.array_equal(zh, z[a:b]) and np.array_equal(Rh, R[a:b]), s
    print(f"{name}: {n_valid} of {N} valid, {n_zero} query points with z == 0, {n_zero_valid} of them valid, {n_flips} flips")
    assert n_valid > N // 4 and n_flips <= 1 and n_zero >= 200 and n_zero_valid >= 50, (n_valid, n_flips, n_zero, n_zero_valid)
    close(g, o)


# ============================================================================= 3. one bucket with insert
@pytest.mark.parametrize("name", ["tilt", "vs04", "layers3", "all"])
def test_update_points_bucket_ladder(oracle_lib, hip_lib, name):
    """test_update_points_bucket_and_insert, then the size ladder of test_update_points_edge_cases (no match, after no match, single
    match, pile of 90 into one voxel, 1, 63, 64, 65, 257 points): counts, intensities, state, covariance, times and map."""
    sc, o, g, xs, Ps, tp = matured(name, oracle_lib, hip_lib, live=True)
    ts = tp + 0.01
    xb = scenes.xyz_of(offconfig.ZeroZ()(sc, ts, 77))[:1500]
    (wo, io_, neo), (wg, ig, neg) = o.update_points(ts, xb), g.update_points(ts, xb)
    assert neo == neg and neo > 100, (neo, neg)
    assert np.array_equal(io_, ig) and np.abs(wo - wg).max() < 1e-5
    (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
    assert np.allclose(xg, xo, rtol=1e-9, atol=1e-10), np.abs(xg - xo).max()
    assert rel_err(Pg, Po) < 1e-7 and o.get_times() == g.get_times()
    scenes.compare_maps(o.map_export(), g.map_export())
    rng = np.random.default_rng(4242)
    ds = scenes.xyz_of(offconfig.ZeroZ()(sc, ts + 0.01, 55))
    far = (rng.uniform(-1, 1, (40, 3)) + np.array([300.0, -200.0, 50.0])).astype(np.float32)
    pile = (np.array([310.0, -210.0, 40.0]) + rng.uniform(0.02, 0.23, (90, 3))).astype(np.float32)
    cases = [("no match", far), ("after no match", ds[:700]), ("single match", None), ("pile > 64 into one voxel", pile), ("one point", ds[700:701]),
             ("63", ds[701:764]), ("64", ds[764:828]), ("65", ds[828:893]), ("257", ds[893:1150])]
    t = ts
    seen_zero = seen_one = False
    for case, xb in cases:
        t += 0.004
        if xb is None:
            valid = o.residuals(ds[1150:])[3]
            k = 1150 + int(np.flatnonzero(valid)[0])
            xb = np.concatenate([ds[k:k + 1], far[:5] + 7.0])
        (wo, io_, neo), (wg, ig, neg) = o.update_points(t, xb), g.update_points(t, xb)
        assert neo == neg, (case, neo, neg)
        seen_zero |= neo == 0
        seen_one |= neo == 1
        assert np.array_equal(io_, ig), case
        assert np.abs(wo - wg).max() < 2e-4, (case, np.abs(wo - wg).max())
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-9), (case, np.abs(xg - xo).max())
        assert rel_err(Pg, Po) < 1e-7, case
        assert o.get_times() == g.get_times(), case
    assert seen_zero and seen_one
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-7)
    close(g, o)


def test_update_points_on_the_corner_sites_deep4(oracle_lib, hip_lib):
    """Three buckets of `fresh` site points through lk_update_points on the five-level corner-site map: insert into, refit and freeze
    of leaves on layers 3 and 4; compare_maps after each bucket."""
    sc, o, g = make_pair("deep4", oracle_lib, hip_lib)
    blob = site_blob("deep4", oracle_lib)
    x = site_state()
    o.close()
    o = site_oracle("deep4", oracle_lib)     # live: see matured()
    g.map_import(blob)
    for obj in (o, g):
        obj.set_state(x, 1e-6 * np.eye(30))
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
        obj.set_times(1.0, 1.0)
    before = offconfig.layer_counts(scenes.canon_map(blob))
    for k in range(3):
        xs, _ = o.get_state()
        xb = site_queries(sc.P, xs, 20 + k, n_per_sheet=60)
        t = 1.0 + 0.002 * (k + 1)
        (wo, io_, neo), (wg, ig, neg) = o.update_points(t, xb), g.update_points(t, xb)
        assert neo == neg and neo > 300, (k, neo, neg)
        assert np.array_equal(io_, ig) and np.abs(wo - wg).max() < 1e-5
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-9), (k, np.abs(xg - xo).max())
        assert rel_err(Pg, Po) < 1e-7, k
        scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-7)
    after = offconfig.layer_counts(scenes.canon_map(g.map_export()))
    print("deep4 buckets: nodes / planes per layer before", before, "after", after)
    close(g, o)


# ============================================================================= 4. whole scans, every stream kernel
@pytest.mark.parametrize("use_kin", [False, True])
@pytest.mark.parametrize("name", offconfig.CLOSED_LOOP)
def test_sequence_scan_resident_and_launches(oracle_lib, hip_lib, name, use_kin):
    sequence_scan_resident_and_launches(oracle_lib, hip_lib, name, use_kin)


def sequence_scan_resident_and_launches(oracle_lib, hip_lib, name, use_kin, scene=None, n_scans=6):
    """test_sequence_imu_mode / test_sequence_kin_mode / test_scan_resident_kernel_equals_per_bucket_launches: first frame + 6
    recorded-shape scans through the scan-resident kernel and through the per-bucket launches (lk_stream_resident(0)): the two
    bit-identical (state, covariance, re-projected cloud, map), both equal to the oracle - bucket / update / match counts exact on
    every scan, state to 1e-7 (IMU-only) or rtol 1e-7 / atol 1e-8 (leg fusion) as in those tests, map as in test_sequence_imu_mode."""
    sc, o, g = make_pair(name, oracle_lib, hip_lib, use_kin=use_kin, scene=scene)
    g_pb = hip_lib.LegKiloHip(sc.cfg())
    g_pb.stream_resident(False)
    t0 = 2.0
    for obj in (o, g, g_pb):
        x0 = scenes.init_filter(obj, sc, t0)
        scenes.first_frame(obj, sc, t0, x0)
    zin = offconfig.ZeroZ()
    for k in range(n_scans):
        tb = t0 + 0.1 * k
        ds = zin(sc, tb, k)
        kw = dict(kins=synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=3003 + k)) if use_kin else \
            dict(imus=synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k))
        po, _ = o.process_scan(ds, tb, **kw)
        pg, wg = g.process_scan(ds, tb, want_world=True, **kw)
        pp, wp = g_pb.process_scan(ds, tb, want_world=True, **kw)
        assert (po.n_buckets, po.n_updates, int(po.n_effect)) == (pg.n_buckets, pg.n_updates, int(pg.n_effect)) == \
            (pp.n_buckets, pp.n_updates, int(pp.n_effect)), (k, po.n_effect, pg.n_effect, pp.n_effect)
        assert po.n_buckets > 100 and po.n_effect > 300, (k, po.n_buckets, po.n_effect)
        (xo, _), (xg, Pg), (xp, Pp) = o.get_state(), g.get_state(), g_pb.get_state()
        if use_kin:    # test_sequence_kin_mode
            assert np.allclose(xo, xg, rtol=1e-7, atol=1e-8), (k, np.abs(xo - xg).max())
        else:          # test_scan_resident_kernel_equals_per_bucket_launches (all 36 entries; test_sequence_imu_mode asks 1e-7 of the position)
            assert np.abs(xo - xg).max() < 1e-7, (k, np.abs(xo - xg).max())
        assert np.array_equal(xg, xp) and np.array_equal(Pg, Pp), (k, np.abs(xg - xp).max())
        assert np.array_equal(wg, wp), k
    scenes.maps_identical(g.map_export(), g_pb.map_export())
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-6)
    n_res, n_relaunch = g.stream_resident_stats()
    print(f"{name} use_kin={use_kin}: scan-resident kernel ran {n_res} scans, {n_relaunch} launches beyond one per scan; z == 0 path points {zin.n_zero}")
    assert n_res == n_scans and g_pb.stream_resident_stats()[0] == 0, (n_res, g_pb.stream_resident_stats())
    close(g, g_pb, o)


@pytest.mark.parametrize("nb", [5, 51])
@pytest.mark.parametrize("name", ["tilt", "all"])
def test_scan_grid_kernel_and_launches(oracle_lib, hip_lib, name, nb):
    scan_grid_kernel_and_launches(oracle_lib, hip_lib, name, nb)


def scan_grid_kernel_and_launches(oracle_lib, hip_lib, name, nb, scene=None):
    """test_scan_grid_kernel_equals_per_bucket_launches, reduced (two scans of 30 000 points in 5 buckets / 70 000 in 51 two-ms bins:
    the kernel takes scans whose smallest bucket holds more than 512 points): the grid-resident kernel against the per-bucket
    launches bit for bit, both against the oracle (counts exact, state 1e-6, same voxels)."""
    sc, o, g = make_pair(name, oracle_lib, hip_lib, scene=scene)
    g_seq = hip_lib.LegKiloHip(sc.cfg())
    g.stream_grid(2)
    g_seq.stream_grid(0)
    g_seq.stream_resident(False)
    t0 = 13.0
    for obj in (o, g, g_seq):
        x0 = scenes.init_filter(obj, sc, t0)
        scenes.first_frame(obj, sc, t0, x0, dense=20000)
    for k in range(2):
        tb = t0 + 0.1 * k
        pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=70000 if nb == 51 else 30000, n_buckets=nb, seed_scan=9300 + k, seed_noise=9400 + k)
        pts["z"][::37] = 0.0
        po, _ = o.process_scan(pts, tb)
        pg, wg = g.process_scan(pts, tb, want_world=True)
        ps, ws = g_seq.process_scan(pts, tb, want_world=True)
        assert (po.n_buckets, po.n_updates, int(po.n_effect)) == (pg.n_buckets, pg.n_updates, int(pg.n_effect)) == (ps.n_buckets, ps.n_updates, int(ps.n_effect)), \
            (k, po.n_effect, pg.n_effect, ps.n_effect)
        assert po.n_buckets == nb and po.n_effect > 2000
        (xo, _), (xg, Pg), (xs, Ps) = o.get_state(), g.get_state(), g_seq.get_state()
        assert np.abs(xo - xg).max() < 1e-6, (k, np.abs(xo - xg).max())
        assert np.array_equal(xg, xs) and np.array_equal(Pg, Ps), (k, np.abs(xg - xs).max())
        assert np.array_equal(wg, ws), k
    scenes.maps_identical(g.map_export(), g_seq.map_export())
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-6)
    n_scans, n_relaunch = g.stream_resident_stats()
    print(f"{name} grid-resident kernel, {nb} buckets: {n_scans} scans, {n_relaunch} launches beyond one per scan")
    assert n_scans == 2 and g_seq.stream_resident_stats()[0] == 0, (n_scans, g_seq.stream_resident_stats())
    close(g, g_seq, o)


# ============================================================================= 5. batch replay on the frozen map
def frozen_replay(g, scans, xs, Ps):
    S, n_pts = len(scans), len(scans[0])
    off, dt = synth.buckets_of(scans[0])
    for s_ in scans:
        o2, d2 = synth.buckets_of(s_)
        assert np.array_equal(o2, off) and np.array_equal(d2, dt)
    allpts = np.concatenate(scans)
    d_pts = g.device_malloc(allpts.nbytes)
    g.h2d(d_pts, allpts)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    poses = g.batch_replay_dev(d_pts, S, n_pts, 0.0, off, dt)
    g.device_free(d_pts)
    X, Pc = g.batch_get_states(0, S)
    return poses, np.array(X), np.array(Pc)


def check_frozen_replay(o, scans, xs, Ps, poses, X, Pc, least_effect):
    """test_batch_replay_frozen_map's comparison of every slot with the oracle's frozen-map replay."""
    o.set_map_insert(False)
    for s in range(len(scans)):
        o.set_state(xs[s], Ps[s])
        o.set_times(0.0, 0.0)
        po, _ = o.process_scan(scans[s], 0.0)
        xo, Po = o.get_state()
        assert (po.n_buckets, po.n_updates, po.n_effect) == (poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect), \
            (s, po.n_effect, poses[s].n_effect)
        assert po.n_effect > least_effect, (s, po.n_effect)
        assert np.allclose(xo, X[s], rtol=1e-8, atol=1e-9), (s, np.abs(xo - X[s]).max())
        assert np.allclose(np.array(poses[s].pos), xo[9:12], atol=1e-8)
        assert np.abs(Pc[s].reshape(30, 30) - Po).max() <= 1e-6 * np.abs(Po).max(), s


def grid_off_handle(hip_lib, cfg, monkeypatch):
    monkeypatch.setenv("LEGKILO_GRID", "0")
    try:
        return hip_lib.LegKiloHip(cfg)
    finally:
        monkeypatch.delenv("LEGKILO_GRID")


@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_batch_replay_frozen_map(oracle_lib, hip_lib, monkeypatch, name):
    """test_batch_replay_frozen_map (S = 6): lk_batch_replay_dev on the frozen-map grid and with LEGKILO_GRID=0 (hash lookups) - the
    two bit-identical, both against the oracle's frozen-map replay of every slot."""
    S, n_pts, nb = 6, 8000, 5
    sc, o, g, xs0, Ps0, tp = matured(name, oracle_lib, hip_lib, n_slots=S)
    rng = np.random.default_rng(5005)
    xs, Ps, scans = [], [], []
    for s in range(S):
        tb = tp + 0.2 + 0.37 * s
        sc_ = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=n_pts, n_buckets=nb, seed_scan=5005 + s, seed_noise=6006 + s)
        sc_["z"][::37] = 0.0
        scans.append(sc_)
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
    poses, X, Pc = frozen_replay(g, scans, xs, Ps)
    check_frozen_replay(o, scans, xs, Ps, poses, X, Pc, least_effect=1000)
    g0 = grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch)
    g0.map_import(g.map_export())
    g0.init_process_cov_q()
    poses0, X0, Pc0 = frozen_replay(g0, scans, xs, Ps)
    assert np.array_equal(X0, X) and np.array_equal(Pc0, Pc)
    assert [int(p.n_effect) for p in poses0] == [int(p.n_effect) for p in poses]
    close(g0, g, o)


@pytest.mark.parametrize("name", ["deep4", "deep3"])
def test_batch_replay_frozen_corner_sites(oracle_lib, hip_lib, monkeypatch, name):
    """The frozen-map replay on the corner-site map: 6 slots with perturbed priors, 3 buckets of `fresh` site points each - the grid's
    flattened candidate lists (planes of layers 1 .. 4 behind a non-plane root) against the tree walk (LEGKILO_GRID=0) against the
    oracle."""
    S = 6
    sc, o, g = make_pair(name, oracle_lib, hip_lib, n_slots=S)
    blob = site_blob(name, oracle_lib)
    for obj in (o, g):
        obj.map_import(blob)
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
    xs = [site_state(s) for s in range(S)]
    Ps = [1e-6 * np.eye(30) for _ in range(S)]
    scans = [offconfig.deal_buckets(site_queries(sc.P, xs[s], 30 + s, n_per_sheet=80), 3) for s in range(S)]
    poses, X, Pc = frozen_replay(g, scans, xs, Ps)
    check_frozen_replay(o, scans, xs, Ps, poses, X, Pc, least_effect=900)
    g0 = grid_off_handle(hip_lib, sc.cfg(n_slots=S), monkeypatch)
    g0.map_import(blob)
    g0.init_process_cov_q()
    g0.set_acc_norm(9.81)
    poses0, X0, Pc0 = frozen_replay(g0, scans, xs, Ps)
    assert np.array_equal(X0, X) and np.array_equal(Pc0, Pc)
    assert [int(p.n_effect) for p in poses0] == [int(p.n_effect) for p in poses]
    print(f"{name}: frozen replay n_effect per slot {[int(p.n_effect) for p in poses]}")
    close(g0, g, o)


# ============================================================================= 8. -0.0 in ext_R: generic kernels, identity arithmetic
def test_negzero_generic_kernels_equal_the_specialised_ones(oracle_lib, hip_lib):
    """A handle created with ext_R = [1, -0.0, 0, ...] takes the generic instantiations (ext_identity is a bit compare) and must
    give results np.array_equal to a handle created with the shipped configuration in the same process: lk_residuals,
    lk_update_points, lk_process_scan (scan-resident, IMU-only) and lk_batch_replay_dev."""
    S = 6
    blob, xs0, Ps0, (tp, tu) = mature_blob(None, oracle_lib)
    out = []
    for name in (None, "negzero"):
        sc = offconfig.scene(name, **CAPS)
        g = hip_lib.LegKiloHip(sc.cfg(n_slots=S))
        g.map_import(np.frombuffer(blob, dtype=np.uint8))
        g.set_state(xs0, Ps0)
        g.init_process_cov_q()
        g.set_acc_norm(9.81)
        g.set_times(tp, tu)
        res = {}
        ts = tp + 0.3
        pts = synth.dense_scan(sc.world, scenes.Frozen(sc.traj, ts), ts, sc.P, n=20000, n_buckets=1)
        pts["z"][::37] = 0.0
        res["residuals"] = g.residuals(scenes.xyz_of(pts))
        rng = np.random.default_rng(5005)
        xs, Ps, scans = [], [], []
        for s in range(S):
            tb = tp + 0.2 + 0.37 * s
            scans.append(synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=8000, n_buckets=5, seed_scan=5005 + s, seed_noise=6006 + s))
            xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
            Ps.append(1e-4 * np.eye(30))
        poses, X, Pc = frozen_replay(g, scans, xs, Ps)
        res["replay"] = (X, Pc, np.array([int(p.n_effect) for p in poses]))
        g.set_state(xs0, Ps0)
        g.set_times(tp, tu)
        xb = scenes.xyz_of(offconfig.ZeroZ()(sc, tp + 0.01, 77))[:1500]
        w, inten, ne = g.update_points(tp + 0.01, xb)
        res["update_points"] = (w, inten, np.array(ne), *g.get_state())
        seq = []
        for k in range(3):
            tb = tp + 0.1 * (k + 1)
            ds = offconfig.ZeroZ()(sc, tb, 20 + k)
            pose, w = g.process_scan(ds, tb, imus=synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k), want_world=True)
            seq += [w, np.array([pose.n_buckets, pose.n_updates, pose.n_effect]), *g.get_state()]
        assert g.stream_resident_stats()[0] == 3
        res["process_scan"] = tuple(seq)
        res["map"] = bytes(g.map_export())
        out.append(res)
        g.close()
    a, b = out
    assert a["residuals"][3].sum() > 1000 and int(a["update_points"][2]) > 100 and a["replay"][2].min() > 1000
    for key in ("residuals", "replay", "update_points", "process_scan"):
        for i, (u, v) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(u, v), (key, i)
    scenes.maps_identical(np.frombuffer(a["map"], dtype=np.uint8), np.frombuffer(b["map"], dtype=np.uint8))


# ============================================================================= 6. batch replay with insert
def overlay_replay_and_check(o, g, tag, blob, scans, xs, Ps, reserve, least_effect):
    """lk_batch_replay_overlay_dev + lk_overlay_export against the oracle's KILO::process on a private copy of the map, slot by slot
    (test_batch_replay_overlay): counts exact, state 1e-6, covariance 1e-6, compare_overlay for every slot; the shared map untouched;
    a second replay gives the same bits."""
    S, n_pts = len(scans), len(scans[0])
    base = scenes.canon_map(blob)
    off, dt = synth.buckets_of(scans[0])
    for s_ in scans:
        o2, d2 = synth.buckets_of(s_)
        assert np.array_equal(o2, off) and np.array_equal(d2, dt)
    allpts = np.concatenate(scans)
    d_pts = g.device_malloc(allpts.nbytes)
    g.h2d(d_pts, allpts)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    n_eff_frozen = [int(p.n_effect) for p in g.batch_replay_dev(d_pts, S, n_pts, 0.0, off, dt)]
    g.overlay_reserve(*reserve)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    poses = g.batch_replay_overlay_dev(d_pts, S, n_pts, 0.0, off, dt)
    Xall, Pall = g.batch_get_states(0, S)
    scenes.maps_identical(g.map_export(), blob)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    poses2 = g.batch_replay_overlay_dev(d_pts, S, n_pts, 0.0, off, dt)
    X2, P2 = g.batch_get_states(0, S)
    assert np.array_equal(Xall, X2) and np.array_equal(Pall, P2)
    assert [int(p.n_effect) for p in poses] == [int(p.n_effect) for p in poses2]
    g.device_free(d_pts)
    differs = 0
    for s in range(S):
        o.map_import(blob)
        o.set_map_insert(True)
        o.set_state(xs[s], Ps[s])
        o.set_times(0.0, 0.0)
        po, _ = o.process_scan(scans[s], 0.0)
        xo, Po = o.get_state()
        assert (po.n_buckets, po.n_updates, int(po.n_effect)) == (poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect)), \
            (tag, s, po.n_effect, poses[s].n_effect, n_eff_frozen[s])
        assert po.n_effect > least_effect, (tag, s, po.n_effect)
        assert np.abs(xo - Xall[s]).max() < 1e-6, (tag, s, np.abs(xo - Xall[s]).max())
        assert np.abs(Pall[s] - Po).max() <= 1e-6 * np.abs(Po).max(), (tag, s)
        st = scenes.compare_overlay(g.overlay_export(s), base, scenes.canon_map(o.map_export()), (tag, s), rtol=1e-5, ptol=1e-7)
        assert st["private_roots"] > 0 and st["changed_roots"] > 0, (tag, s, st)
        differs += int(int(po.n_effect) != n_eff_frozen[s])
        print(f"overlay {tag} slot {s}: n_effect {int(po.n_effect)} (frozen map: {n_eff_frozen[s]}), private roots {st['private_roots']}, "
              f"changed by the oracle {st['changed_roots']}, nodes compared {st.get('nodes', 0)}, max |dx| {np.abs(xo - Xall[s]).max():.2e}")
    return differs


@pytest.mark.parametrize("name", ["tilt", "vs04", "layers3", "all"])
def test_batch_replay_overlay_scattered(oracle_lib, hip_lib, name):
    batch_replay_overlay_scattered(oracle_lib, hip_lib, name)


def batch_replay_overlay_scattered(oracle_lib, hip_lib, name, scene=None):
    """Case `scattered` of test_batch_replay_overlay at its own size (4 slots x 30 000 points): the buckets are a random partition of the
    scan on a young map, so every bucket's insert refits / creates planes the next bucket matches."""
    S, n_pts, nb = 4, 30000, 5
    sc, o, g = make_pair(name, oracle_lib, hip_lib, scene=scene, n_slots=S)
    t0 = 21.0
    x0 = scenes.init_filter(o, sc, t0)
    scenes.first_frame(o, sc, t0, x0, dense=20000)
    o.map_import(o.map_export())     # the form a blob round trip leaves the map in (dead points of cut inner nodes are not carried)
    blob = o.map_export()
    g.map_import(blob)
    g.init_process_cov_q()
    rng = np.random.default_rng(515151)
    xs, Ps, scans = [], [], []
    for s in range(S):
        tb = t0 + 0.5 + 0.21 * s
        pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=n_pts, n_buckets=nb, seed_scan=7005 + s, seed_noise=7106 + s)
        curv = pts["curvature"].copy()
        pts = pts[rng.permutation(len(pts))]
        pts["curvature"] = curv
        pts["z"][::37] = 0.0
        scans.append(pts)
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
    differs = overlay_replay_and_check(o, g, name, blob, scans, xs, Ps, (16384, 32768, 16384), least_effect=1000)
    assert differs == S, (differs, S)     # the insert really changed what later buckets matched
    close(g, o)


def test_batch_replay_overlay_corner_sites_deep4(oracle_lib, hip_lib):
    """lk_batch_replay_overlay_dev on the corner-site map at max_layer 4: 6 slots, 3 buckets of `fresh` site points each - whole
    five-level octrees are copied on write and refitted privately."""
    S = 6
    sc, o, g = make_pair("deep4", oracle_lib, hip_lib, n_slots=S)
    o.map_import(site_blob("deep4", oracle_lib))
    blob = o.map_export()
    g.map_import(blob)
    for obj in (o, g):
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
    xs = [site_state(s) for s in range(S)]
    Ps = [1e-6 * np.eye(30) for _ in range(S)]
    scans = [offconfig.deal_buckets(site_queries(sc.P, xs[s], 40 + s, n_per_sheet=80), 3) for s in range(S)]
    overlay_replay_and_check(o, g, "deep4", blob, scans, xs, Ps, (4096, 65536, 65536), least_effect=900)
    close(g, o)


@pytest.mark.parametrize("name", ["tilt", "vs04", "layers3", "all"])
def test_batch_replay_overlay_ragged_scan_resident_imu(oracle_lib, hip_lib, monkeypatch, name):
    batch_replay_overlay_ragged_scan_resident_imu(oracle_lib, hip_lib, monkeypatch, name)


def batch_replay_overlay_ragged_scan_resident_imu(oracle_lib, hip_lib, monkeypatch, name, scene=None):
    """Mode `imu` of test_batch_replay_overlay_ragged_scan_resident: lk_batch_replay_overlay_ragged_dev in its scan-resident form and
    launch by launch (LEGKILO_RAG_RESIDENT=0) on a young map - the same bits, and per slot the oracle's KILO::process on a private copy
    of the map: counts exact, state 1e-6, private voxels equal.  Shapes: config-1 scans (one with volumetric clutter), 40 buckets of
    ~150 points, a one-point scan."""
    sc = scene or offconfig.scene(name, **CAPS)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    t0 = 2.0
    x0 = scenes.init_filter(o, sc, t0)
    scenes.first_frame(o, sc, t0, x0)
    o.map_import(o.map_export())
    blob = o.map_export()
    base = scenes.canon_map(blob)
    rng = np.random.default_rng(717171)
    shapes = [None, (6000, 40), "clutter", (1, 1)]
    zin = offconfig.ZeroZ()
    scans, tbs, xs, Ps, msgs = [], [], [], [], []
    for s, shp in enumerate(shapes):
        tb = t0 + 0.4 + 0.23 * s
        x_prior = synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5)
        if shp is None:
            pts = zin(sc, tb, 180 + s)
        elif shp == "clutter":
            pts = zin(sc, tb, 180 + s)
            pw = scenes.corner_clutter(rng, n_cells=30, per_cell=60, origin=tuple(x_prior[9:12] + np.array([1.5, -1.0, -0.2])))
            pb = offconfig.body_of(x_prior, pw, sc.P)
            cl = offconfig.deal_buckets(pb, 1)
            stamps = np.unique(pts["curvature"])
            cl["curvature"] = stamps[((np.arange(len(pb)) // 60) * (len(stamps) // 31)) % len(stamps)]
            pts = np.concatenate([pts, cl])
            pts = pts[np.argsort(pts["curvature"], kind="stable")]
        else:
            pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=shp[0], n_buckets=shp[1], seed_scan=7600 + s, seed_noise=7700 + s)
        assert np.diff(synth.buckets_of(pts)[0].astype(np.int64)).max() <= 512
        scans.append(pts), tbs.append(tb), xs.append(x_prior), Ps.append(1e-4 * np.eye(30))
        msgs.append(synth.imu_stream(sc.traj, tb, tb + 0.1, seed=9500 + s))
    S = len(scans)
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=S))
    g.map_import(blob)
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    o.set_acc_norm(9.81)
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    poses = g.batch_replay_overlay_ragged(scans, tbs, xs, Ps, imus=msgs)
    rounds = g.overlay_resident_rounds()
    Xall, Pall = g.batch_get_states(0, S)
    exports = [g.overlay_export(s) for s in range(S)]
    assert rounds >= 1, "the scan-resident form did not run"
    for s in range(S):
        o.map_import(blob)
        o.set_map_insert(True)
        o.set_state(xs[s], Ps[s])
        o.set_times(tbs[s], tbs[s])
        po, _ = o.process_scan(scans[s], tbs[s], imus=msgs[s])
        xo, Po = o.get_state()
        assert (po.n_buckets, po.n_updates, int(po.n_effect)) == (poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect)), \
            (name, s, po.n_buckets, po.n_updates, po.n_effect, poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect)
        assert np.abs(xo - Xall[s]).max() < 1e-6, (name, s, np.abs(xo - Xall[s]).max())
        assert np.abs(Pall[s] - Po).max() <= 1e-6 * np.abs(Po).max(), (name, s)
        st = scenes.compare_overlay(exports[s], base, scenes.canon_map(o.map_export()), (name, s), rtol=1e-4, ptol=2e-6)
        print(f"scan-resident overlay {name} slot {s}: {len(scans[s])} points, {po.n_buckets} buckets, n_effect {int(po.n_effect)}, "
              f"private roots {st['private_roots']}, max |dx| {np.abs(xo - Xall[s]).max():.2e}; {rounds} launches")
    monkeypatch.setenv("LEGKILO_RAG_RESIDENT", "0")
    poses0 = g.batch_replay_overlay_ragged(scans, tbs, xs, Ps, imus=msgs)
    assert g.overlay_resident_rounds() == 0
    X0, P0 = g.batch_get_states(0, S)
    assert np.array_equal(Xall, X0) and np.array_equal(Pall, P0), "scan-resident and launch-by-launch replay differ"
    for s in range(S):
        assert (poses0[s].n_buckets, poses0[s].n_updates, int(poses0[s].n_effect)) == (poses[s].n_buckets, poses[s].n_updates, int(poses[s].n_effect))
        assert scenes.maps_identical(g.overlay_export(s), exports[s]), (name, s)
    close(g, o)


# ============================================================================= 7. around the path
def count_tree(blob_bytes):
    """(nodes, point blocks) reachable from the roots of a blob."""
    def walk(n):
        nn, nb = 1, 1 if n["pts"] is not None else 0
        for c in n["children"].values():
            a, b = walk(c)
            nn, nb = nn + a, nb + b
        return nn, nb

    tot = [walk(n) for n in scenes.canon_map(blob_bytes).values()]
    return sum(t[0] for t in tot), sum(t[1] for t in tot)


def test_slide_compaction_and_checkpoint_closed_loop_all(oracle_lib, hip_lib, tmp_path):
    """test_map_sliding_parity_and_compaction + test_checkpoint_resume_is_bit_identical at configuration `all`: same slide decision and
    surviving map as the oracle, pools compacted to the live four-level trees, the path keeps running on them; a checkpoint restored
    into a fresh handle continues bit-identically."""
    from legkilo_amd import checkpoint

    sc, o, g = make_pair("all", oracle_lib, hip_lib)
    t0 = 1.0
    for obj in (o, g):
        x0 = scenes.init_filter(obj, sc, t0)
        scenes.first_frame(obj, sc, t0, x0)
    ro = scenes.replay_vlp(o, sc, t0, 3)
    rg = scenes.replay_vlp(g, sc, t0, 3)
    roots0, nodes0, blocks0 = g.map_stats()
    pos = rg[-1][1][9:12]
    so = o.map_slide(ro[-1][1][9:12], sliding_thresh=0.0, half_map_size=8)
    sg = g.map_slide(pos, sliding_thresh=0.0, half_map_size=8)
    assert so == sg and sg[0] and 0 < sg[1] < roots0, (so, sg, roots0)
    blob_g = g.map_export()
    scenes.compare_maps(o.map_export(), blob_g, rtol=1e-6, ptol=1e-7)
    roots1, nodes1, blocks1 = g.map_stats()
    assert roots1 == roots0 - sg[1] and (nodes1, blocks1) == count_tree(blob_g) and nodes1 < nodes0
    checkpoint.save(tmp_path / "ck.npz", g)
    b = hip_lib.LegKiloHip(sc.cfg())
    checkpoint.restore(tmp_path / "ck.npz", b)
    ro2 = scenes.replay_vlp(o, sc, t0, 3, start=3)
    rg2 = scenes.replay_vlp(g, sc, t0, 3, start=3)
    rb2 = scenes.replay_vlp(b, sc, t0, 3, start=3)
    for k, ((po, xo), (pg, xg), (pb, xb)) in enumerate(zip(ro2, rg2, rb2)):
        assert (po.n_buckets, po.n_updates, po.n_effect) == (pg.n_buckets, pg.n_updates, pg.n_effect) == (pb.n_buckets, pb.n_updates, pb.n_effect), k
        assert np.allclose(xo, xg, rtol=1e-7, atol=1e-8), (k, np.abs(xo - xg).max())
        assert np.array_equal(xg, xb), (k, np.abs(xg - xb).max())
    assert np.array_equal(g.get_state()[1], b.get_state()[1])
    scenes.compare_maps(g.map_export(), b.map_export(), rtol=0.0, ptol=0.0)
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-6, ptol=1e-6)
    vs = float(np.float32(sc.P["voxel_size"]))
    k = np.floor(pos / vs).astype(int)
    box = (k[0] + 3, k[0] - 6, k[1] + 5, k[1] - 2, k[2] + 8, k[2] - 8)
    assert o.map_clear_outside(*box) == g.map_clear_outside(*box)
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-6, ptol=1e-6)
    close(b, g, o)


def test_slide_compaction_and_checkpoint_corner_sites_deep4(oracle_lib, hip_lib, tmp_path):
    """The same around the five-level trees of the corner-site + uniform-box map: slide (roots of whole sites removed, pools compacted
    to the live nodes of all five layers), then buckets of `fresh` site points on the compacted pools, on the handle and on a fresh
    handle restored from a checkpoint - bit-identical to each other, equal to the oracle."""
    from legkilo_amd import checkpoint

    sc, o, g = make_pair("deep4", oracle_lib, hip_lib)
    o.close()
    o = site_oracle("deep4", oracle_lib)
    g.map_import(site_blob("deep4", oracle_lib))
    x = site_state()
    for obj in (o, g):
        obj.set_state(x, 1e-6 * np.eye(30))
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
        obj.set_times(1.0, 1.0)
    roots0, nodes0, blocks0 = g.map_stats()
    centre = np.array([14.0, -1.0, 0.7])      # keeps the sites within 8 m (16 voxels) of it, drops the others
    so, sg = o.map_slide(centre, 0.0, 16), g.map_slide(centre, 0.0, 16)
    assert so == sg and sg[0] and 0 < sg[1] < roots0, (so, sg, roots0)
    blob_g = g.map_export()
    scenes.compare_maps(o.map_export(), blob_g, rtol=1e-6, ptol=1e-9)
    roots1, nodes1, blocks1 = g.map_stats()
    assert roots1 == roots0 - sg[1] and (nodes1, blocks1) == count_tree(blob_g) and nodes1 < nodes0
    nodes, _ = offconfig.layer_counts(scenes.canon_map(blob_g))
    assert (nodes > 0).all(), nodes
    checkpoint.save(tmp_path / "ck.npz", g)
    b = hip_lib.LegKiloHip(sc.cfg())
    checkpoint.restore(tmp_path / "ck.npz", b)
    for k in range(2):
        xs, _ = o.get_state()
        pw, _ = sites().fresh(50 + k, 60)
        keep = np.abs(pw - centre).max(1) < 7.0          # points of the sites that survived the slide
        xb = offconfig.body_of(xs, pw[keep], sc.P)
        t = 1.0 + 0.002 * (k + 1)
        (wo, io_, neo), (wg, ig, neg), (wb, ib, neb) = o.update_points(t, xb), g.update_points(t, xb), b.update_points(t, xb)
        assert neo == neg == neb and neo > 200, (k, neo, neg, neb)
        (xo, Po), (xg, Pg), (xb_, Pb) = o.get_state(), g.get_state(), b.get_state()
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-9), (k, np.abs(xg - xo).max())
        assert np.array_equal(xg, xb_) and np.array_equal(Pg, Pb) and np.array_equal(wg, wb), k
    scenes.compare_maps(g.map_export(), b.map_export(), rtol=0.0, ptol=0.0)
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=1e-7)
    close(b, g, o)


# ============================================================================= 5 (continued). voxel order and ragged batches
@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_batch_sort_by_voxel(oracle_lib, hip_lib, name):
    """test_batch_sort_by_voxel (its explicit part): lk_batch_sort_by_voxel_dev keys every point with THIS configuration's extrinsic and
    voxel size - afterwards every bucket holds exactly its own points, the 64 points of a residual tile lie in far fewer root voxels
    (counted here with scenes.world_of and the double voxel size), and the replay of the sorted batch equals the oracle's replay of
    the same sorted scans (counts exact, state rtol 1e-8 / atol 1e-9)."""
    S, n_pts, nb = 6, 8000, 5
    sc, o, g, xs0, Ps0, tp = matured(name, oracle_lib, hip_lib, n_slots=S)
    o.set_map_insert(False)
    rng = np.random.default_rng(6116)
    xs, Ps, scans = [], [], []
    for s in range(S):
        tb = tp + 0.2 + 0.37 * s
        sc_ = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=n_pts, n_buckets=nb, seed_scan=6116 + s, seed_noise=7227 + s)
        off, dt = synth.buckets_of(sc_)
        for b in range(nb):
            a, e = int(off[b]), int(off[b + 1])
            sc_[a:e] = sc_[a:e][rng.permutation(e - a)]
        scans.append(sc_)
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
    off, dt = synth.buckets_of(scans[0])
    allpts = np.ascontiguousarray(np.concatenate(scans))
    d_in, d_out = g.device_malloc(allpts.nbytes), g.device_malloc(allpts.nbytes)
    g.h2d(d_in, allpts)
    g.batch_set_priors(np.array(xs), np.array(Ps))
    g.batch_sort_by_voxel_dev(d_in, d_out, S, n_pts, off)
    srt = np.empty_like(allpts)
    g.d2h(srt, d_out)
    vs = float(sc.P["voxel_size"])

    def voxels_per_tile(sc_, x_):
        cnt = []
        for b in range(nb):
            a, e = int(off[b]), int(off[b + 1])
            key = np.floor(scenes.world_of(x_, scenes.xyz_of(sc_[a:e]), sc.P).astype(np.float64) / vs).astype(np.int64)
            lin = (key[:, 2] * 4096 + key[:, 1]) * 4096 + key[:, 0]
            cnt += [len(np.unique(lin[i:i + 64])) for i in range(0, e - a, 64)]
        return float(np.mean(cnt))

    for s in range(S):
        a_in, a_out = allpts[s * n_pts:(s + 1) * n_pts], srt[s * n_pts:(s + 1) * n_pts]
        for b in range(nb):
            a, e = int(off[b]), int(off[b + 1])
            u_in, u_out = (np.ascontiguousarray(q[a:e]).view(np.uint64).reshape(-1, 2) for q in (a_in, a_out))
            assert np.array_equal(u_in[np.lexsort((u_in[:, 1], u_in[:, 0]))], u_out[np.lexsort((u_out[:, 1], u_out[:, 0]))]), (s, b)
        v_in, v_out = voxels_per_tile(a_in, xs[s]), voxels_per_tile(a_out, xs[s])
        assert v_out < 0.7 * v_in, (s, v_in, v_out)
    print(f"{name}: distinct root voxels per 64-point tile: {voxels_per_tile(allpts[:n_pts], xs[0]):.1f} in random order, {voxels_per_tile(srt[:n_pts], xs[0]):.1f} sorted")
    poses = g.batch_replay_dev(d_out, S, n_pts, 0.0, off, dt)
    for s in range(S):
        o.set_state(xs[s], Ps[s])
        o.set_times(0.0, 0.0)
        po, _ = o.process_scan(srt[s * n_pts:(s + 1) * n_pts], 0.0)
        xo, _ = o.get_state()
        xg, _ = g.get_state(slot=s)
        assert (po.n_buckets, po.n_updates, po.n_effect) == (poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect), s
        assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xg).max())
    g.device_free(d_in)
    g.device_free(d_out)
    close(g, o)


@pytest.mark.parametrize("name", ["tilt", "vs04", "all"])
def test_batch_replay_ragged_and_scans(oracle_lib, hip_lib, name):
    """test_batch_replay_ragged reduced to 4 scans (8 000 points in 5 buckets, a config-1 scan of ~370 buckets, 65 points in one bucket,
    one point): lk_batch_replay_ragged_dev against the oracle's bucket loop over each scan alone, lk_batch_replay_scans_dev (bucket
    tables built on the device) bit-identical to it, and both again with the IMU messages between the buckets."""
    blob, xs0, Ps0, (tp, tu) = mature_blob(name, oracle_lib)
    sc, o, g = make_pair(name, oracle_lib, hip_lib, n_slots=4)
    for obj in (o, g):
        obj.map_import(np.frombuffer(blob, dtype=np.uint8))
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
    o.set_map_insert(False)
    rng = np.random.default_rng(8118)
    scans, tbs, xs, Ps = [], [], [], []
    for s, shp in enumerate([(8000, 5), None, (65, 1), (1, 1)]):
        tb = tp + 0.1 + 0.23 * s
        if shp is None:
            sc_ = offconfig.ZeroZ()(sc, tb, 40 + s)
        else:
            sc_ = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=shp[0], n_buckets=shp[1], seed_scan=8200 + s, seed_noise=8300 + s)
        scans.append(sc_), tbs.append(tb), Ps.append(1e-4 * np.eye(30))
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
    d_all = g.device_malloc(sum(s_.nbytes for s_ in scans))
    for with_imu in (False, True):
        # messages between the buckets are replayed for scans whose buckets hold <= 512 points: the dense 5-bucket scan stays out of that pass
        pick = [1, 2, 3] if with_imu else [0, 1, 2, 3]
        sub, stb, sx, sP = [scans[i] for i in pick], [tbs[i] for i in pick], [xs[i] for i in pick], [Ps[i] for i in pick]
        imus = [synth.imu_stream(sc.traj, tb_, tb_ + 0.1, seed=8600 + s) for s, tb_ in enumerate(stb)]
        kw = dict(imus=imus) if with_imu else {}
        poses = g.batch_replay_ragged(sub, stb, sx, sP, host_tables=True, **kw)
        first = []
        for s in range(len(sub)):
            o.set_state(sx[s], sP[s])
            o.set_times(stb[s], stb[s])
            po, _ = o.process_scan(sub[s], stb[s], **(dict(imus=imus[s]) if with_imu else {}))
            xo, Po = o.get_state()
            xg, Pg = g.get_state(slot=s)
            assert (po.n_buckets, po.n_updates, po.n_effect) == (poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect), (with_imu, s)
            assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (with_imu, s, np.abs(xo - xg).max())
            assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (with_imu, s, np.abs(Po - Pg).max())
            first.append((poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect, xg, Pg))
        big = [f for f in first if f[0] > 100]
        assert len(big) == 1 and big[0][2] > 300 and (with_imu or first[0][2] > 1000), [f[:3] for f in first]
        allp = np.ascontiguousarray(np.concatenate(sub))
        so = np.r_[0, np.cumsum([len(s_) for s_ in sub])]
        g.h2d(d_all, allp)
        g.batch_set_priors(np.asarray(sx), np.asarray(sP))
        pd = g.batch_replay_scans_dev(d_all, so, stb, **kw)
        for s in range(len(sub)):
            assert (pd[s].n_buckets, pd[s].n_updates, pd[s].n_effect) == first[s][:3], (with_imu, s)
            xd, Pd = g.get_state(slot=s)
            assert np.array_equal(xd, first[s][3]) and np.array_equal(Pd, first[s][4]), (with_imu, s)
    g.device_free(d_all)
    close(g, o)
