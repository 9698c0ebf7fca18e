"""The frozen-grid residual kernels request a point's cell record BEFORE they compute the point-only terms (lk_point_kernels.h, residual_tile
with GRID == 1) and match the cell's own record from the registers the request filled.  What that order could get wrong, on the smallest shapes:

* tiles with lanes beyond the bucket's end - buckets of 1, 63, 64, 65 and 130 points through the uniform and the ragged entry: such lanes must
  request nothing and contribute zero rows;
* single tiles that mix every way a first look-up can end: plane cell, outside the grid's bounding box, empty cell, list header with zero
  records, list header with several records, home plane failed and the neighbour retry matched, body point with z == 0.

Expected values, none of them from the code under test: the oracle's match count per bucket (exact) and state (tolerances of
test_gpu_parity.py's batch tests), and the same call on a handle with the grid switched off (LEGKILO_GRID=0: the hash-table instantiation, whose
order of operations is the old one) bit for bit.  Every crafted case is first established on the CPU, from the map blob and with the oracle."""
import numpy as np
import pytest

import scenes
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
SIZES = (1, 63, 64, 65, 130)
T0 = 1.0
CASES = ("plane", "outside", "empty", "list0", "list2", "retry", "z0")


# ----------------------------------------------------------------------------- CPU side: the map, its cells, the crafted points
def trunc_key(pw, vs):
    """KILO.cc:143-148: float cast, -1.0 for negatives, (int) truncation."""
    loc = (np.asarray(pw, float) / vs).astype(np.float32)
    loc = np.where(loc < 0, (loc.astype(np.float64) - 1.0).astype(np.float32), loc)
    return loc.astype(np.int64)


def body_of(x36, pw, P):
    R, p = x36[:9].reshape(3, 3), x36[9:12]
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    return (((np.asarray(pw, float) - p) @ R - T) @ E).astype(np.float32)


def world_of(x36, xb, P):
    """The world point in fp64 (KILO.cc:126-131) of float body points."""
    R, p = x36[:9].reshape(3, 3), x36[9:12]
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    return (np.asarray(xb, np.float64) @ E.T + T) @ R.T + p


def point_var(oracle_lib, x36, P30, xb, P):
    """KILO.cc:132-140: the world covariance of one body point."""
    R = x36[:9].reshape(3, 3)
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    pb = np.asarray(xb, np.float64)
    body = np.asarray(oracle_lib.calc_body_cov(pb, float(P["dept_err"]), float(P["beam_err"]))).reshape(3, 3)
    pi = E @ pb + T
    K = np.array([[0, -pi[2], pi[1]], [pi[2], 0, -pi[0]], [-pi[1], pi[0], 0]])
    RE, RK = R @ E, R @ K
    return RE @ body @ RE.T + RK @ P30[:3, :3] @ RK.T + P30[3:6, 3:6]


def roots_of(blob):
    """key -> (root is a plane, plane records of its subtree in pre-order) of every root voxel of a map blob."""
    b = abi.parse_blob(blob)
    nodes, planes = b["nodes"], b["planes"]
    out = {}
    for r in b["roots"]:
        top = int(r["node"])
        rec, stack = [], [top]
        while stack:
            i = stack.pop()
            if planes[i]["flags"] & abi.LK_PLANE_IS_PLANE:
                rec.append(planes[i])
                continue
            stack += [int(k) for k in nodes[i]["child"][::-1] if k >= 0]
        out[tuple(int(k) for k in r["key"])] = (bool(planes[top]["flags"] & abi.LK_PLANE_IS_PLANE), rec)
    return out


class Case:
    pass


@pytest.fixture(scope="module")
def case(oracle_lib):
    """One oracle map (first frame, four scans, clutter that cuts voxels), one prior, and per kind of first look-up a pool of body points
    whose kind the oracle and the blob confirm."""
    c = Case()
    c.sc = sc = scenes.Scene(**CAPS)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    scenes.mature_oracle_map(o, sc, T0, n_scans=4)
    centre = sc.traj.pos(T0 + 1.3)
    clutter = scenes.corner_clutter(np.random.default_rng(77), n_cells=40, per_cell=80, origin=(centre[0] + 2.0, centre[1] - 1.0, 3.0))
    o.map_update(clutter, np.tile((1e-4 * np.eye(3)).reshape(1, 9), (len(clutter), 1)))
    c.blob = o.map_export()
    o.set_map_insert(False)
    c.x0 = x0 = synth.initial_state(sc.traj, T0 + 1.3, sc.P)
    c.P0 = P0 = 1e-4 * np.eye(30)
    o.set_state(x0, P0)
    P, vs = sc.P, float(sc.P["voxel_size"])
    roots = roots_of(c.blob)
    keys = np.array(list(roots))
    kmin, kmax = keys.min(0), keys.max(0)
    rng = np.random.default_rng(2024)

    def confirmed(pw, want_key_in, want_valid):
        """Body points of world points pw whose truncated key satisfies want_key_in and whose oracle verdict is want_valid."""
        xb = body_of(x0, pw, P)
        k = trunc_key(world_of(x0, xb, P), vs)
        ok = np.array([want_key_in(tuple(int(v) for v in kk)) for kk in k])
        v = o.residuals(xb)[3].astype(bool)
        return xb[ok & (v == want_valid)]

    pools = {}
    # plane cells: the centre of a root plane, a little off along the plane
    pl = [(k, r[1][0]) for k, r in roots.items() if r[0]]
    pw = np.array([np.array(p["center"], float) for _, p in pl])
    pools["plane"] = confirmed(pw, lambda k: k in roots and roots[k][0], True)
    # outside the bounding box of the root keys, on every side
    out = []
    for ax in range(3):
        for kk in (kmin[ax] - 3, kmax[ax] + 3):
            k = ((kmin + kmax) // 2).astype(float)
            k[ax] = kk
            out.append((k + 0.5) * vs)
    pools["outside"] = confirmed(np.array(out), lambda k: bool(np.any(np.array(k) < kmin) or np.any(np.array(k) > kmax)), False)
    # empty cells: keys inside the box without a root
    emp = []
    while len(emp) < 64:
        k = rng.integers(kmin, kmax + 1)
        if tuple(int(v) for v in k) not in roots:
            emp.append((k + 0.5) * vs)
    inside = lambda k: bool(np.all(np.array(k) >= kmin) and np.all(np.array(k) <= kmax))   # noqa: E731
    pools["empty"] = confirmed(np.array(emp), lambda k: inside(k) and k not in roots, False)
    # list headers: roots that are no plane, with no plane below them / with two or more
    l0 = np.array([(np.array(k) + 0.5) * vs for k, r in roots.items() if not r[0] and len(r[1]) == 0])
    pools["list0"] = confirmed(l0, lambda k: k in roots and not roots[k][0] and len(roots[k][1]) == 0, False) if len(l0) else np.zeros((0, 3), np.float32)
    l2 = np.array([np.array(p["center"], float) for k, r in roots.items() if not r[0] and len(r[1]) >= 2 for p in r[1]])
    pools["list2"] = confirmed(l2, lambda k: k in roots and not roots[k][0] and len(roots[k][1]) >= 2, True)
    # neighbour retry: points of a root plane's support that lie just across the border of its voxel, in a voxel that exists; kept where the
    # oracle matches the point although its home voxel alone (match_voxel) does not
    cand = []
    for k, p in pl:
        cc, n = np.array(p["center"], float), np.array(p["normal"], float)
        lo = np.array(k) * vs
        for _ in range(6):
            d = rng.normal(size=3)
            d -= n * (d @ n)
            d /= np.linalg.norm(d)
            t = np.where(d > 0, (lo + vs - cc) / np.where(d > 0, d, 1), np.where(d < 0, (lo - cc) / np.where(d < 0, d, -1), np.inf)).min()
            cand.append(cc + (t + 0.02) * d)
    xb = confirmed(np.array(cand), lambda k: k in roots, True)
    keep = []
    for b in xb:
        w = world_of(x0, b, P)
        m = o.match_voxel(trunc_key(w, vs).astype(np.int32), w, point_var(oracle_lib, x0, P0, b, P).reshape(9))
        if m["found"] and not m["success"]:
            keep.append(b)
        if len(keep) == 16:
            break
    pools["retry"] = np.array(keep, np.float32).reshape(-1, 3)
    # body points with z == 0 exactly that the oracle matches: rays in the sensor's own horizontal plane
    az = rng.uniform(0, 2 * np.pi, 48)
    r = np.arange(1.5, 20.0, 0.01)
    zb = np.stack([np.outer(np.cos(az), r).ravel(), np.outer(np.sin(az), r).ravel(), np.zeros(len(az) * len(r))], 1).astype(np.float32)
    zb = zb[o.residuals(zb)[3].astype(bool)]
    pools["z0"] = zb[rng.permutation(len(zb))[:64]]
    for name in CASES:
        assert len(pools[name]) >= 2, (name, len(pools[name]))
    assert np.all(pools["z0"][:, 2] == 0.0)
    print("crafted pools:", {k: len(v) for k, v in pools.items()})
    c.pools, c.o = pools, o
    yield c
    o.close()


def scan_of(xb, sizes):
    """Body points as a scan whose buckets have the given sizes (curvature steps of 1 us: the state hardly moves between them)."""
    assert len(xb) == sum(sizes)
    scan = np.zeros(len(xb), dtype=synth.POINT_DTYPE)
    scan["x"], scan["y"], scan["z"] = xb[:, 0], xb[:, 1], xb[:, 2]
    scan["curvature"] = np.repeat(np.arange(len(sizes), dtype=np.float32) * np.float32(1e-6), sizes)
    off, dt = synth.buckets_of(scan)
    assert np.array_equal(np.diff(off.astype(np.int64)), sizes)
    return scan, off, dt


def mixed_tiles(c, n, seed):
    """n body points in which EVERY aligned run of 64 holds every kind of CASES at least once (the rest: plane cells and list records)."""
    rng = np.random.default_rng(seed)
    fill = np.concatenate([c.pools["plane"], c.pools["list2"]])
    xb = fill[rng.integers(0, len(fill), n)].copy()
    for t0 in range(0, n, 64):
        m = min(64, n - t0)
        if m < len(CASES):
            continue
        lanes = rng.permutation(m)[: 2 * len(CASES)]
        for j, lane in enumerate(lanes):
            pool = c.pools[CASES[j % len(CASES)]]
            xb[t0 + lane] = pool[rng.integers(0, len(pool))]
    return xb


def oracle_scan(c, scan, t_begin=0.0):
    o = c.o
    o.set_state(c.x0, c.P0)
    o.set_times(t_begin, t_begin)
    po, _ = o.process_scan(scan, t_begin)
    xo, Po = o.get_state()
    return (int(po.n_buckets), int(po.n_updates), int(po.n_effect)), xo.copy(), Po.copy()


def oracle_count(c, xb):
    """Matches of body points under the prior (one bucket): the oracle's valid mask."""
    c.o.set_state(c.x0, c.P0)
    return int(c.o.residuals(xb)[3].sum())


def handles(hip_lib, monkeypatch, c, n_slots):
    """(name, handle) with the frozen grid on and off; the caller closes them."""
    for name, env in (("grid", None), ("pool", "0")):
        monkeypatch.delenv("LEGKILO_GRID", raising=False)
        if env is not None:
            monkeypatch.setenv("LEGKILO_GRID", env)
        g = hip_lib.LegKiloHip(c.sc.cfg(n_slots=n_slots))
        g.map_import(c.blob)
        g.init_process_cov_q()
        yield name, g
        g.close()
    monkeypatch.delenv("LEGKILO_GRID", raising=False)


def check_against_oracle(tag, got, want):
    (cnt_g, xg, Pg), (cnt_o, xo, Po) = got, want
    assert cnt_g == cnt_o, (tag, cnt_g, cnt_o)
    assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (tag, np.abs(xo - xg).max())
    assert np.abs(Pg - Po).max() <= 1e-6 * np.abs(Po).max(), (tag, np.abs(Pg - Po).max() / np.abs(Po).max())


# ----------------------------------------------------------------------------- GPU side
def test_uniform_entry_bucket_sizes_and_mixed_tiles(case, hip_lib, monkeypatch):
    """lk_batch_replay_dev (lk_residual_kernel<false, 1, *>): one bucket of 1, 63, 64, 65, 130 points, each tile mixing every kind of first
    look-up, then the five as ONE scan of five buckets."""
    c = case
    runs = [mixed_tiles(c, n, 100 + n) for n in SIZES]
    scans = [scan_of(xb, [len(xb)]) for xb in runs] + [scan_of(np.concatenate(runs), list(SIZES))]
    want = []
    for xb, (scan, off, dt) in zip(runs + [None], scans):
        w = oracle_scan(c, scan)
        if xb is not None:   # a single bucket: its match count is the count of the oracle's valid mask under the prior
            assert w[0] == (1, 1 if oracle_count(c, xb) > 0 else 0, oracle_count(c, xb)), (len(xb), w[0])
        want.append(w)
    assert sum(w[0][2] for w in want[:-1]) > 0 and want[-1][0][0] == len(SIZES)
    res = {}
    for name, g in handles(hip_lib, monkeypatch, c, 2):
        res[name] = []
        for scan, off, dt in scans:
            both = np.concatenate([scan, scan])   # two slots, the same scan: the second slot's tiles start at another workgroup
            d_pts = g.device_malloc(both.nbytes)
            g.h2d(d_pts, both)
            g.batch_set_priors(np.array([c.x0, c.x0]), np.array([c.P0, c.P0]))
            poses = g.batch_replay_dev(d_pts, 2, len(scan), 0.0, off, dt)
            X, P = g.batch_get_states(0, 2)
            g.device_free(d_pts)
            assert np.array_equal(X[0], X[1]) and np.array_equal(P[0], P[1])
            assert (poses[0].n_buckets, poses[0].n_updates, poses[0].n_effect) == (poses[1].n_buckets, poses[1].n_updates, poses[1].n_effect)
            res[name].append(((int(poses[0].n_buckets), int(poses[0].n_updates), int(poses[0].n_effect)), X[0].copy(), P[0].copy()))
    for k, w in enumerate(want):
        tag = SIZES[k] if k < len(SIZES) else "chain"
        print("uniform", tag, "oracle", w[0], "grid", res["grid"][k][0], "pool", res["pool"][k][0])
        check_against_oracle(("uniform", tag), res["grid"][k], w)
        assert res["grid"][k][0] == res["pool"][k][0], tag
        assert np.array_equal(res["grid"][k][1], res["pool"][k][1]) and np.array_equal(res["grid"][k][2], res["pool"][k][2]), tag


def test_ragged_entry_bucket_sizes_and_mixed_tiles(case, hip_lib, monkeypatch):
    """lk_residual_ragged_kernel<1> (the per-bucket launches of the ragged entry, LEGKILO_RAGGED_LEVELS=1): five scans of one bucket of 1, 63,
    64, 65, 130 points in ONE launch - the grid is sized for 130, so every smaller scan has whole workgroups and partial tiles beyond its end -
    and a sixth scan that chains the five sizes as buckets."""
    c = case
    runs = [mixed_tiles(c, n, 200 + n) for n in SIZES]
    scans = [scan_of(xb, [len(xb)])[0] for xb in runs] + [scan_of(np.concatenate(runs), list(SIZES))[0]]
    S = len(scans)
    tbs = [0.0] * S
    want = [oracle_scan(c, sc_) for sc_ in scans]
    for xb, w in zip(runs, want):
        assert w[0][2] == oracle_count(c, xb), (len(xb), w[0])
    monkeypatch.setenv("LEGKILO_RAGGED_LEVELS", "1")
    res = {}
    for name, g in handles(hip_lib, monkeypatch, c, S):
        poses = g.batch_replay_ragged(scans, tbs, [c.x0] * S, [c.P0] * S, host_tables=True)
        X, P = g.batch_get_states(0, S)
        res[name] = [((int(poses[s].n_buckets), int(poses[s].n_updates), int(poses[s].n_effect)), X[s].copy(), P[s].copy()) for s in range(S)]
    monkeypatch.delenv("LEGKILO_RAGGED_LEVELS")
    for s in range(S):
        tag = SIZES[s] if s < len(SIZES) else "chain"
        print("ragged", tag, "oracle", want[s][0], "grid", res["grid"][s][0], "pool", res["pool"][s][0])
        check_against_oracle(("ragged", tag), res["grid"][s], want[s])
        assert res["grid"][s][0] == res["pool"][s][0], tag
        assert np.array_equal(res["grid"][s][1], res["pool"][s][1]) and np.array_equal(res["grid"][s][2], res["pool"][s][2]), tag


def test_each_kind_of_first_lookup_alone(case, hip_lib, monkeypatch):
    """A bucket of 64 points of ONE kind per slot (seven slots, one launch): the oracle's count is all of them for the kinds that match and
    none for the kinds that have no plane to match - a prefetched header taken for a plane, or a retry that evaluates the header, shows here."""
    c = case
    rng = np.random.default_rng(7)
    runs = [c.pools[name][rng.integers(0, len(c.pools[name]), 64)] for name in CASES]
    _, off, dt = scan_of(runs[0], [64])   # every slot's bucket table
    scans = [scan_of(xb, [64])[0] for xb in runs]
    want = [oracle_scan(c, sc_) for sc_ in scans]
    for name, w in zip(CASES, want):
        assert w[0][2] == (64 if name in ("plane", "list2", "retry", "z0") else 0), (name, w[0])
    S = len(CASES)
    allpts = np.concatenate(scans)
    res = {}
    for hname, g in handles(hip_lib, monkeypatch, c, S):
        d_pts = g.device_malloc(allpts.nbytes)
        g.h2d(d_pts, allpts)
        g.batch_set_priors(np.array([c.x0] * S), np.array([c.P0] * S))
        poses = g.batch_replay_dev(d_pts, S, 64, 0.0, off, dt)
        X, P = g.batch_get_states(0, S)
        g.device_free(d_pts)
        res[hname] = [((int(poses[s].n_buckets), int(poses[s].n_updates), int(poses[s].n_effect)), X[s].copy(), P[s].copy()) for s in range(S)]
    for s, name in enumerate(CASES):
        print("kind", name, "oracle", want[s][0], "grid", res["grid"][s][0], "pool", res["pool"][s][0])
        check_against_oracle(("kind", name), res["grid"][s], want[s])
        assert res["grid"][s][0] == res["pool"][s][0], name
        assert np.array_equal(res["grid"][s][1], res["pool"][s][1]) and np.array_equal(res["grid"][s][2], res["pool"][s][2]), name
