"""-m gpu: lk_overlay_commit - one slot's insert overlay of the last replay with insert becomes part of the handle's map, on the device - against
the CPU oracle's map after KILO::process of that slot's scans on a private copy of the base map.

The scene is test_overlay_runs.py's (its helpers are imported, the file is not changed): a young map from a first frame, blob round-tripped; six
runs of 3 / 1 / 4 / 2 / 1 / 3 config-1 scans, some with clutter; priors from synth.initial_state(..., 0.02, 0.5), P = 1e-4 I; modes plain / imu /
kin.  It produces split leaves, lazily copied voxels, cut voxels and voxels the base map lacks.  Map tolerances are those of that file for the
same kernels on the same scene (rtol 1e-4, ptol 2e-6), counts are exact, poses 1e-6, the final state of a chain of scans CHAIN_XTOL.  A mode's
scans, its handle and the oracle's results are computed once and shared; every test restores the handle's map with map_import(blob) first.
"""
import numpy as np
import pytest

import scenes
import test_overlay_runs as tor
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

CAPS, MODES, T0, SCAN_GAP, CHAIN_XTOL = tor.CAPS, tor.MODES, tor.T0, tor.SCAN_GAP, tor.CHAIN_XTOL
COMMIT = (0, 2, 5)   # a run with clutter, the four-scan run with the one-point scan, a run ending in clutter
RTOL, PTOL = 1e-4, 2e-6
ERR_INVALID, ERR_CAPACITY, ERR_STATE = r"error -1:", r"error -3:", r"error -5:"
P0 = 1e-4 * np.eye(30)


def msg_kw(mode, m):
    return {} if mode == "plain" else {"imus" if mode == "imu" else "kins": m}


def oracle_run(o, blob, x, P, run, tb_run, mode, msgs):
    """tor.oracle_run, with the oracle's map afterwards as a BLOB (scenes.compare_maps takes blobs); the oracle keeps that map."""
    poses, xo, Po, _ = tor.oracle_run(o, blob, x, P, run, tb_run, mode, msgs)
    return poses, xo, Po, o.map_export()


def oracle_scans(o, scans, tbs, mode, msgs, x, P):
    """The oracle goes on from the map it holds: set_state / set_times(tb, tb) as oracle_run does at a run's start, then scan after scan."""
    o.set_map_insert(True)
    o.set_state(x, P)
    o.set_times(tbs[0], tbs[0])
    out = []
    for j, (pts, tb) in enumerate(zip(scans, tbs)):
        po, _ = o.process_scan(pts, tb, **msg_kw(mode, None if msgs is None else msgs[j]))
        out.append(((po.n_buckets, po.n_updates, int(po.n_effect)), np.array(po.rot), np.array(po.pos), np.array(po.vel)))
    return out, o.get_state()[0].copy()


def build_case(mode, oracle_lib, hip_lib, scene_plain):
    sc, o, blob = tor.young_map(oracle_lib, mode, scene_plain)
    o.set_acc_norm(9.81)
    rng = np.random.default_rng(828282)   # the scans and priors of tor.oracle_side, draw for draw
    runs, tbs, xs, k = [], [], [], 0
    for r, shapes in enumerate(tor.RUN_SHAPES):
        tb0 = T0 + 0.4 + 0.23 * r
        tb_run = [tb0 + SCAN_GAP * j for j in range(len(shapes))]
        run = []
        for shp, tb in zip(shapes, tb_run):
            run.append(tor.make_scan(sc, rng, shp, tb, k))
            k += 1
        runs.append(run)
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb0, sc.P, rng, 0.02, 0.5))
    msgs = tor.run_messages(sc, mode, runs, tbs)
    c = dict(mode=mode, sc=sc, o=o, blob=blob, base=scenes.canon_map(blob), runs=runs, tbs=tbs, xs=xs, msgs=msgs)
    # the scan after run 5 (test 6): the oracle goes on live from its post-run map and state
    tb_next = tbs[5][-1] + SCAN_GAP
    c["next"] = (tor.make_scan(sc, rng, None, tb_next, 99), tb_next, None if mode == "plain" else tor.stream(sc, mode, tb_next, 99))
    c["after"] = {}
    for r in COMMIT:
        c["after"][r] = oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], mode, None if msgs is None else msgs[r])
        if r == 5:
            pts, tb, m = c["next"]
            po, _ = o.process_scan(pts, tb, **msg_kw(mode, m))
            c["next_oracle"] = ((po.n_buckets, po.n_updates, int(po.n_effect)), np.array(po.rot), np.array(po.pos), np.array(po.vel))
    c["g"] = new_handle(hip_lib, c)
    return c


def new_handle(hip_lib, c, **over):
    g = hip_lib.LegKiloHip(c["sc"].cfg(n_slots=len(c["runs"]), **over))
    g.map_import(c["blob"])
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    return g


@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()
        c["o"].close()


@pytest.fixture(params=MODES)
def case(request, built, oracle_lib, hip_lib, scene_plain, monkeypatch):
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    if request.param not in built:
        built[request.param] = build_case(request.param, oracle_lib, hip_lib, scene_plain)
    return built[request.param]


def fresh_replay(c, g=None):
    """The base map back, then one call of the runs entry from the case's priors."""
    g = c["g"] if g is None else g
    g.map_import(c["blob"])
    return tor.device_call(g, c)


def same_voxel(a, b, where):
    """scenes.maps_identical's comparison of one voxel: bit for bit, node ids aside."""
    for f in ("layer", "npts", "new_points", "is_plane", "state", "quater"):
        assert a[f] == b[f], (where, f, a[f], b[f])
    assert np.array_equal(a["center"], b["center"]), (where, "center")
    if a["is_plane"]:
        for f in ("center", "normal", "d", "radius", "flags", "points_size", "plane_var", "min_ev", "mid_ev", "max_ev"):
            assert np.array_equal(a["plane"][f], b["plane"][f]), (where, "plane", f)
    assert (a["pts"] is None) == (b["pts"] is None), (where, "points presence")
    if a["pts"] is not None:
        assert np.array_equal(a["pts"]["pw"], b["pts"]["pw"]) and np.array_equal(a["pts"]["var"], b["pts"]["var"]), (where, "points")
    assert set(a["children"]) == set(b["children"]), (where, "children")
    for o in a["children"]:
        same_voxel(a["children"][o], b["children"][o], where + (o,))


def reachable(blob):
    """(roots, nodes, point blocks) that the roots of a blob reach, walked in numpy level by level."""
    b = abi.parse_blob(blob)
    nodes = b["nodes"]
    level = np.asarray(b["roots"]["node"], dtype=np.int64)
    all_nodes = []
    while len(level):
        all_nodes.append(level)
        ch = nodes["child"][level].reshape(-1)
        level = ch[ch >= 0].astype(np.int64)
    ids = np.concatenate(all_nodes) if all_nodes else np.zeros(0, dtype=np.int64)
    assert len(np.unique(ids)) == len(ids), "a node is reached twice"
    blk = nodes["block"][ids]
    blk = blk[blk >= 0]
    assert len(np.unique(blk)) == len(blk), "a point block is owned twice"
    return len(b["roots"]), len(ids), len(blk)


def check_no_leak(g, blob, oracle_roots, where):
    """4. lk_map_stats: the oracle's root count, and exactly the nodes and point blocks the exported roots reach."""
    stats = g.map_stats()
    rr = reachable(blob)
    print(f"{where}: lk_map_stats {stats}, reachable in the export {rr}, oracle roots {oracle_roots}")
    assert stats[0] == oracle_roots, (where, stats, oracle_roots)
    assert stats == rr, (where, stats, rr)


def check_committed(c, committed, export, oracle_blob, where):
    """1. The committed map against the oracle's, and bit for bit against the base map (keys the export lacks) and the export (keys it holds)."""
    st = scenes.compare_maps(committed, oracle_blob, rtol=RTOL, ptol=PTOL)   # (asserts that the root key sets are equal)
    A, E, B = scenes.canon_map(committed), scenes.canon_map(export), c["base"]
    assert set(A) == set(B) | set(E), (where, len(A), len(B), len(E))
    kept = new = 0
    for k, v in A.items():
        if k in E:
            same_voxel(v, E[k], (where, "export", k))
            new += int(k not in B)
        else:
            same_voxel(v, B[k], (where, "base", k))
            kept += 1
    print(f"{where}: {st['roots']} roots ({kept} the base map's, {len(E)} the overlay's of which {new} new), {st.get('nodes', 0)} nodes compared")
    assert kept > 0 and new > 0 and len(E) > new, (where, "the scene shows no kept / replaced / added voxel", kept, len(E), new)
    return st


def test_committed_map_is_the_oracles(case):
    """1 + 4. Slots 0, 2 and 5 in turn, each behind map_import(blob) and a fresh replay: compare_maps against the oracle's map after that run
    (root key sets equal), untouched keys bit-identical to the base map, private keys bit-identical to the export; lk_map_stats counts the oracle's
    roots and exactly the reachable records."""
    g = case["g"]
    for r in COMMIT:
        fresh_replay(case)
        export = g.overlay_export(r)
        g.overlay_commit(r)
        committed = g.map_export()
        oracle_blob = case["after"][r][3]
        check_committed(case, committed, export, oracle_blob, (case["mode"], r))
        check_no_leak(g, committed, abi.parse_blob(oracle_blob)["header"].n_roots, (case["mode"], r))


def test_commit_directly_or_export_first(case):
    """2. replay, commit and replay, export, commit give the same map: merging the split leaves is idempotent."""
    g = case["g"]
    for r in COMMIT:
        fresh_replay(case)
        g.overlay_commit(r)
        direct = g.map_export()
        fresh_replay(case)
        g.overlay_export(r)
        g.overlay_commit(r)
        assert scenes.maps_identical(direct, g.map_export()) > 0, (case["mode"], r)


def test_windowed_mapping_continues(case):
    """3 + 4. The four-scan run in two windows of two scans on every slot under different priors; slot r of window 1 is committed, window 2 starts
    from batch_get_states -> batch_set_priors against the committed map.  The oracle keeps its map after window 1 and is armed at the boundary as
    oracle_run arms it at a run's start, with the prior the device is armed with.  Slot r and one other slot (oracle started from the committed
    map) match: counts exact, poses 1e-6, final state CHAIN_XTOL.  The oracle alone shows that window 2 matches differently against the base map."""
    g, o, mode, sc = case["g"], case["o"], case["mode"], case["sc"]
    S, r, s = len(case["runs"]), 1, 4
    run, tb, m = case["runs"][2], case["tbs"][2], None if mode == "plain" else case["msgs"][2]
    rng = np.random.default_rng(31337)
    xs = [synth.initial_state(sc.traj, tb[0], sc.P, rng, 0.02, 0.5) for _ in range(S)]
    g.map_import(case["blob"])
    tor.device_call(g, case, runs=[run[:2]] * S, tbs=[tb[:2]] * S, xs=xs, msgs=None if m is None else [m[:2]] * S)
    X1, P1 = g.batch_get_states(0, S)
    assert len({X1[i].tobytes() for i in range(S)}) == S, "the slots' priors do not tell them apart"
    g.overlay_commit(r)
    committed = g.map_export()
    g.batch_set_priors(X1, P1)
    poses = g.batch_replay_overlay_runs([run[2:]] * S, [tb[2:]] * S, **msg_kw(mode, None if m is None else [m[2:]] * S))
    X2, _ = g.batch_get_states(0, S)

    def check(slot, want, x_want, tag):
        for j, (cnt, rot, pos, vel) in enumerate(want):
            p = poses[slot][j]
            d = max(np.abs(np.array(p.rot) - rot).max(), np.abs(np.array(p.pos) - pos).max(), np.abs(np.array(p.vel) - vel).max())
            print(f"{mode} window 2, {tag} slot {slot} scan {j}: counts {cnt} / device {(p.n_buckets, p.n_updates, int(p.n_effect))}, max |d pose| {d:.2e}")
            assert (p.n_buckets, p.n_updates, int(p.n_effect)) == cnt, (mode, tag, slot, j)
            assert d < 1e-6, (mode, tag, slot, j, d)
        dx = np.abs(x_want - X2[slot]).max()
        print(f"{mode} window 2, {tag} slot {slot}: final max |dx| {dx:.2e}")
        assert dx < CHAIN_XTOL, (mode, tag, slot, dx)

    # slot r: the oracle's own map after window 1
    oracle_run(o, case["blob"], xs[r], P0, run[:2], tb[:2], mode, None if m is None else m[:2])
    want_r, x_r = oracle_scans(o, run[2:], tb[2:], mode, None if m is None else m[2:], X1[r], P1[r])
    oracle_final = o.map_export()
    check(r, want_r, x_r, "committed")
    # slot s: another window-1 state on the committed map
    o.map_import(committed)
    want_s, x_s = oracle_scans(o, run[2:], tb[2:], mode, None if m is None else m[2:], X1[s], P1[s])
    check(s, want_s, x_s, "other")
    # the oracle alone: against the base map window 2 matches differently
    o.map_import(case["blob"])
    want_base, _ = oracle_scans(o, run[2:], tb[2:], mode, None if m is None else m[2:], X1[r], P1[r])
    assert any(a[0][2] != b[0][2] for a, b in zip(want_r, want_base)), "window 2 matches the same against the base map: the commit is not shown"
    # the second commit: the four scans' map, nothing leaked
    g.overlay_commit(r)
    final = g.map_export()
    scenes.compare_maps(final, oracle_final, rtol=RTOL, ptol=PTOL)
    check_no_leak(g, final, abi.parse_blob(oracle_final)["header"].n_roots, (mode, "second commit"))


def test_commit_after_the_uniform_entry(oracle_lib, hip_lib, scene_plain):
    """5a. lk_batch_replay_overlay_dev, 4 scans of test_batch_replay_overlay's `tiny` shape (800 points, 12 buckets, young map): the committed map
    against the oracle's as in test 1."""
    scene, S, n_pts, nb, t0 = scene_plain, 4, 800, 12, 21.0
    o = oracle_lib.Oracle(scene.cfg(), imu_mode_only=True)
    g = hip_lib.LegKiloHip(scene.cfg(n_slots=S))
    x0 = scenes.init_filter(o, scene, t0)
    scenes.first_frame(o, scene, t0, x0, dense=20000)
    o.map_import(o.map_export())
    blob = o.map_export()
    g.init_process_cov_q()
    rng = np.random.default_rng(515151)
    xs, scans = [], []
    for s in range(S):
        tb = t0 + 0.5 + 0.21 * s
        pts = synth.dense_scan(scene.world, scene.traj, tb, scene.P, n=n_pts, n_buckets=nb, seed_scan=7005 + s, seed_noise=7106 + s)
        curv = pts["curvature"].copy()
        pts = pts[rng.permutation(len(pts))]
        pts["curvature"] = curv
        scans.append(pts)
        xs.append(synth.initial_state(scene.traj, tb, scene.P, rng, 0.02, 0.5))
    off, dt = synth.buckets_of(scans[0])
    c = dict(base=scenes.canon_map(blob))
    for s in (1, 3):
        g.map_import(blob)
        g.batch_set_priors(np.array(xs), np.array([P0] * S))
        g.batch_replay_overlay(scans, 0.0, off, dt)
        export = g.overlay_export(s)
        g.overlay_commit(s)
        o.map_import(blob)
        o.set_map_insert(True)
        o.set_state(xs[s], P0)
        o.set_times(0.0, 0.0)
        o.process_scan(scans[s], 0.0)
        check_committed(c, g.map_export(), export, o.map_export(), ("uniform", s))
    g.close()
    o.close()


@pytest.mark.parametrize("case", ["plain"], indirect=True)
def test_commit_after_the_ragged_entry(case):
    """5b. lk_batch_replay_overlay_ragged_dev on the first scans of the six runs: slot 2's committed map is the oracle's after that scan."""
    g, o = case["g"], case["o"]
    scans = [run[0] for run in case["runs"]]
    tbs = [tb[0] for tb in case["tbs"]]
    g.map_import(case["blob"])
    g.batch_replay_overlay_ragged(scans, tbs, case["xs"], [P0] * len(scans))
    export = g.overlay_export(2)
    g.overlay_commit(2)
    oracle_blob = oracle_run(o, case["blob"], case["xs"][2], P0, scans[2:3], tbs[2:3], "plain", None)[3]
    check_committed(case, g.map_export(), export, oracle_blob, ("ragged", 2))


def test_commit_after_either_launch_form_of_the_runs_entry(case, hip_lib, monkeypatch):
    """5c. The runs entry launch by launch (LEGKILO_RAG_RESIDENT=0, set before the handle exists) and run-resident: the committed maps are
    identical."""
    maps = {}
    for form in ("0", None):
        if form is None:
            monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
        else:
            monkeypatch.setenv("LEGKILO_RAG_RESIDENT", form)
        g = new_handle(hip_lib, case)
        try:
            tor.device_call(g, case)
            assert (g.overlay_resident_rounds() == 0) == (form == "0")
            g.overlay_commit(2)
            maps[form] = g.map_export()
        finally:
            g.close()
    assert scenes.maps_identical(maps["0"], maps[None]) > 0


def test_adopt_filter(case):
    """6. Without the flag slot 0 keeps its bits; with LK_COMMIT_ADOPT_FILTER it holds slot r's state, covariance and time stamps bit for bit,
    and one lk_process_scan of the next scan from there is the oracle's continuing from its post-run map and state."""
    g, mode, r = case["g"], case["mode"], 5
    fresh_replay(case)
    x0, Pc0 = g.get_state(0)
    t0 = g.get_times(0)
    g.overlay_commit(r)
    xa, Pa = g.get_state(0)
    assert np.array_equal(xa, x0) and np.array_equal(Pa, Pc0) and g.get_times(0) == t0, "flags 0 touched slot 0"
    fresh_replay(case)
    xr, Pr = g.get_state(r)
    tr = g.get_times(r)
    assert not np.array_equal(xr, x0)
    g.overlay_commit(r, adopt_filter=True)
    xa, Pa = g.get_state(0)
    assert np.array_equal(xa, xr) and np.array_equal(Pa, Pr) and g.get_times(0) == tr
    xk, Pk = g.get_state(r)
    assert np.array_equal(xk, xr) and np.array_equal(Pk, Pr), "the committed slot itself changed"
    pts, tb, m = case["next"]
    p, _ = g.process_scan(pts, tb, **msg_kw(mode, m))
    cnt, rot, pos, vel = case["next_oracle"]
    d = max(np.abs(np.array(p.rot) - rot).max(), np.abs(np.array(p.pos) - pos).max(), np.abs(np.array(p.vel) - vel).max())
    print(f"{mode} live scan behind the commit: counts {cnt} / device {(p.n_buckets, p.n_updates, int(p.n_effect))}, max |d pose| {d:.2e}")
    assert (p.n_buckets, p.n_updates, int(p.n_effect)) == cnt
    assert d < 1e-6, d


def test_refusals(case, hip_lib):
    """7. Every refusal leaves lk_map_export byte-equal; after a successful commit the next replay with insert and lk_map_slide work."""
    mode, R = case["mode"], len(case["runs"])

    def refused(g, pattern, call):
        before = g.map_export().tobytes()
        with pytest.raises(hip_lib.LegKiloError, match=pattern):
            call()
        assert g.map_export().tobytes() == before, pattern

    g = new_handle(hip_lib, case)
    try:
        refused(g, ERR_STATE, lambda: g.overlay_commit(0))                      # before any overlay replay
        tor.device_call(g, case)
        refused(g, ERR_INVALID, lambda: g.overlay_commit(R))                    # slot == n_runs
        refused(g, ERR_INVALID, lambda: g.overlay_commit(0, flags=2))
        g.map_update(np.array([[0.3, 0.2, 0.1]]), 1e-4 * np.eye(3).reshape(1, 9))
        refused(g, ERR_STATE, lambda: g.overlay_commit(0))                      # the map has changed since the replay
        fresh_replay(case, g)
        g.overlay_commit(2)
        refused(g, ERR_STATE, lambda: g.overlay_commit(2))                      # a second commit
        refused(g, ERR_STATE, lambda: g.overlay_commit(3))
        refused(g, ERR_STATE, lambda: g.overlay_export(2))
        # the handle goes on: a replay with insert against the committed map, a commit of it, a slide
        tor.device_call(g, case)
        g.overlay_commit(0)
        roots = g.map_stats()[0]
        keys = abi.parse_blob(g.map_export())["roots"]["key"]
        centre = (np.median(keys, axis=0) + 0.5) * float(case["sc"].cfg().max_voxel_size)   # a box of 9 x 9 x 9 voxels in the middle of the map
        slid, removed = g.map_slide(centre, sliding_thresh=0.0, half_map_size=4)
        assert slid and 0 < removed < roots, (slid, removed, roots)
        assert g.map_stats() == reachable(g.map_export())
        tor.device_call(g, case)
        g.overlay_commit(1)
        assert g.map_stats() == reachable(g.map_export())
    finally:
        g.close()
    # pools with room for 8 more records than the base map holds: run 2 needs more (shown on the oracle alone)
    g = new_handle(hip_lib, case)
    _, n_nodes, n_blocks = g.map_stats()
    g.close()
    assert abi.parse_blob(case["after"][2][3])["header"].n_nodes > abi.parse_blob(case["blob"])["header"].n_nodes + 8
    g = new_handle(hip_lib, case, max_roots=n_nodes + 8, max_nodes=n_nodes + 8, max_point_blocks=n_blocks + 8)   # (lk_create wants max_nodes >= max_roots)
    try:
        tor.device_call(g, case)
        refused(g, ERR_CAPACITY + r".*needs \d+ nodes.*max_nodes " + str(n_nodes + 8), lambda: g.overlay_commit(2))
        assert scenes.maps_identical(g.map_export(), case["blob"]) > 0
    finally:
        g.close()
