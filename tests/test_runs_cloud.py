"""-m gpu: lk_batch_replay_runs_cloud_dev / lk_batch_replay_overlay_runs_cloud_dev - the run replays with what KILO::process returns beside the pose:
the state after every time bucket (lk_runs_bucket_poses) and the scans registered into the world frame, every bucket's points under its own state.

The cases are those of test_replay_runs.py (frozen map, mature map) and test_overlay_runs.py (insert, young map with clutter): six runs of 3, 1, 4,
2, 1, 3 scans, a one-point scan in the middle of a run, a 40-bucket dense scan, leftover and looked-back messages at the scan boundaries, modes
plain / imu / kin.  Per entry and mode the borrowed case (the EXISTING entry on its handle, the oracle's passes with their sensitivity assertions) is
built once, and beside it a twin handle that went through the _cloud entry; the checks read those and leave them unchanged.

Tolerances.  Records against what the entry returns: bits.  Cloud against the records (numpy's products against the device's spelled-out FMAs): the
two doubles may straddle a float32 rounding boundary - one float32 ulp.  Cloud against the oracle: those files' per-scan pose bound 1e-6 applied to
every bucket's rotation and position, 1e-6 (1 + |x_i| + |y_i| + |z_i|) with p_i = ext_R p + ext_t, plus one float32 ulp of the oracle's coordinate.
"""
import numpy as np
import pytest

import devguard
import scenes
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

MODES = tor.MODES
KINDS = ["frozen", "overlay"]
P0 = trr.P0
REC = abi.bucket_pose_dtype()
STATE, INVALID = "error -5: ", "error -1: "


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("LEGKILO_RAGGED_LEVELS", "LEGKILO_RAG_RESIDENT", "LEGKILO_POISON_POOLS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def store():
    st = {"trr": {}, "tor": {}, "twin": {}}
    yield st
    for c in list(st["trr"].values()) + list(st["tor"].values()) + list(st["twin"].values()):
        c["g"].close()


def flat(nest):
    return None if nest is None else [x for run in nest for x in run]


def cloud_call(g, kind, mode, runs, tbs, xs, msgs, cont=False):
    """One call of a _cloud entry through the convenience -> everything it leaves: poses, slots, cloud, bucket table."""
    kw = dict(tor.msg_kw(mode, msgs), cloud=True, bucket_poses=True)
    pri = (None, None) if cont else (xs, [P0] * len(runs))
    if kind == "frozen":
        poses, ex = g.batch_replay_runs(runs, tbs, *pri, cont=cont, **kw)
    else:
        poses, ex = g.batch_replay_overlay_runs(runs, tbs, *pri, **kw)
    X, P = g.batch_get_states(0, len(runs))
    return dict(poses=poses, X=X, P=P, times=trr.times_of(g, len(runs)), cloud=ex["cloud"], rec=ex["bucket_poses"], sbo=ex["scan_bucket_off"])


def new_handle(hip_lib, c, n_slots):
    return trr.new_handle(hip_lib, c["sc"], c["blob"], n_slots)


def get_case(kind, mode, store, oracle_lib, hip_lib, scene_plain):
    """The borrowed case `c` (existing entry, oracle) and the twin handle's _cloud call `out`, once per entry and mode."""
    if (kind, mode) not in store["twin"]:
        if kind == "frozen":
            c = trr.build_case(mode, store["trr"], oracle_lib, hip_lib, scene_plain)
        else:
            if mode not in store["tor"]:
                store["tor"][mode] = tor.build_case(mode, oracle_lib, hip_lib, scene_plain)
            c = store["tor"][mode]
        g = new_handle(hip_lib, c, len(c["runs"]))
        out = cloud_call(g, kind, mode, c["runs"], c["tbs"], c["xs"], c["msgs"])
        tw = dict(c=c, g=g, out=out, rounds=g.overlay_resident_rounds(), map=g.map_export().copy())
        if kind == "overlay":
            tw["exports"] = [g.overlay_export(r) for r in range(len(c["runs"]))]
        store["twin"][(kind, mode)] = tw
    return store["twin"][(kind, mode)]


@pytest.fixture(params=[(k, m) for k in KINDS for m in MODES], ids=lambda p: f"{p[0]}-{p[1]}")
def twin(request, store, oracle_lib, hip_lib, scene_plain):
    kind, mode = request.param
    return dict(get_case(kind, mode, store, oracle_lib, hip_lib, scene_plain), kind=kind, mode=mode)


def same_records(a, b, first_point=True):
    fields = [f for f in REC.names if first_point or f != "first_point"]
    return len(a) == len(b) and all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in fields)


def same_cloud(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_records(out, runs, tbs, tag):
    """Check 2: the table against out[], synth.buckets_of on the host copy and the start times."""
    scans, tb, poses = flat(runs), flat(tbs), flat(out["poses"])
    rec, sbo = out["rec"], out["sbo"]
    base, counts = 0, []
    for s, (pts, t0, p) in enumerate(zip(scans, tb, poses)):
        r = rec[int(sbo[s]):int(sbo[s + 1])]
        off, dt = synth.buckets_of(pts)
        counts.append(len(r))
        assert len(r) == p.n_buckets == len(dt), (tag, s, len(r), p.n_buckets, len(dt))
        assert int((r["n_effect"] > 0).sum()) == p.n_updates, (tag, s)
        assert int(r["n_effect"].astype(np.uint64).sum()) == int(p.n_effect), (tag, s)
        assert (r["rot"][-1].tobytes(), r["pos"][-1].tobytes(), r["vel"][-1].tobytes()) == (bytes(p.rot), bytes(p.pos), bytes(p.vel)), (tag, s)
        assert np.array_equal(r["first_point"], base + off[:-1].astype(np.uint64)), (tag, s)
        assert np.array_equal(r["n_points"], np.diff(off.astype(np.int64)).astype(np.uint32)), (tag, s)
        assert r["t"].tobytes() == (np.float64(t0) + dt.astype(np.float64)).tobytes(), (tag, s)
        base += len(pts)
    assert np.array_equal(sbo, np.r_[0, np.cumsum(counts)].astype(np.uint32)), tag
    assert len(rec) == int(sbo[-1])


def body_in_imu(sc, pts):
    eR = np.asarray(sc.P["extrinsic_R"], dtype=np.float64).reshape(3, 3)
    eT = np.asarray(sc.P["extrinsic_T"], dtype=np.float64)
    pb = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
    return pb @ eR.T + eT


def ulp32(a):
    return np.spacing(np.abs(a.astype(np.float32))).astype(np.float64)


def check_cloud(out, runs, sc, tag):
    """Check 3: float32(R (ext_R p + ext_t) + pos) restated from the returned records, one float32 ulp; intensity exact."""
    pts = np.concatenate(flat(runs))
    rec, cloud = out["rec"], out["cloud"]
    assert cloud.shape == (len(pts), 4) and int(rec["n_points"].sum()) == len(pts)
    idx = np.repeat(np.arange(len(rec)), rec["n_points"])
    want = np.einsum("nij,nj->ni", rec["rot"][idx].reshape(-1, 3, 3), body_in_imu(sc, pts)) + rec["pos"][idx]
    w32 = want.astype(np.float32)
    got = cloud[:, :3]
    equal = float(np.mean(got == w32))
    d = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print(f"{tag}: {len(pts)} points, {len(rec)} buckets; coordinates bit-equal to the numpy restatement: {100.0 * equal:.4f} %, largest difference {d.max():.3e}")
    assert np.all(np.isfinite(got))
    assert np.all(d <= np.maximum(ulp32(w32), ulp32(got))), (tag, d.max())
    assert np.array_equal(cloud[:, 3], np.where(rec["n_effect"][idx] > 0, np.float32(255.0), np.float32(0.0))), tag


def test_nothing_else_moved(twin):
    """1. Twin handles, one through the existing entry, one through the _cloud entry: out[], states, covariances, times, overlays, map - bit-equal."""
    c, out, kind = twin["c"], twin["out"], twin["kind"]
    if kind == "frozen":
        assert trr.same_bits((out["poses"], out["X"], out["P"], out["times"]), c["dev"])
        assert np.array_equal(twin["map"], c["map_before"])
    else:
        assert tor.pose_bits(out["poses"]) == tor.pose_bits(c["poses"])
        assert np.array_equal(out["X"], c["X"]) and np.array_equal(out["P"], c["P"])
        assert out["times"] == trr.times_of(c["g"], len(c["runs"]))
        for r in range(len(c["runs"])):
            assert scenes.maps_identical(twin["exports"][r], c["exports"][r]), (twin["mode"], r)
        assert np.array_equal(twin["map"], c["g"].map_export())


def test_records_are_what_the_entry_returns(twin):
    """2."""
    check_records(twin["out"], twin["c"]["runs"], twin["c"]["tbs"], (twin["kind"], twin["mode"]))


def test_cloud_is_the_records_applied_to_the_points(twin):
    """3."""
    check_cloud(twin["out"], twin["c"]["runs"], twin["c"]["sc"], f"{twin['kind']} {twin['mode']}")


def test_cloud_against_the_oracle(twin, oracle_lib, scene_plain):
    """4. process_scan(..., want_world=True) scan after scan on the imported blob (frozen: insert off; with insert: test_overlay_runs.py's run).  The
    oracle pass made here must count what the borrowed one counted; the borrowed cases' sensitivity assertions (trr.oracle_side: the insert changes
    the counts; here for the overlay: putting the map back before every scan does) keep the two entries from passing each other's check."""
    c, out, kind, mode = twin["c"], twin["out"], twin["kind"], twin["mode"]
    sc = c["sc"]
    _, o, blob = (trr.mature_map if kind == "frozen" else tor.young_map)(oracle_lib, mode, scene_plain)   # the borrowed case's oracle, made the same way
    assert np.array_equal(np.frombuffer(blob, dtype=np.uint8), np.frombuffer(c["blob"], dtype=np.uint8))
    o.set_acc_norm(9.81)
    worlds = []
    for r, (run, tb_run) in enumerate(zip(c["runs"], c["tbs"])):
        o.map_import(c["blob"])
        o.set_map_insert(kind == "overlay")
        o.set_state(c["xs"][r], P0)
        o.set_times(tb_run[0], tb_run[0])
        for j, (pts, tb) in enumerate(zip(run, tb_run)):
            kw = {} if mode == "plain" else {"imus" if mode == "imu" else "kins": c["msgs"][r][j]}
            po, w = o.process_scan(pts, tb, want_world=True, **kw)
            assert (po.n_buckets, po.n_updates, int(po.n_effect)) == c["oracle"][r][0][j][0], (r, j)
            worlds.append(w)
    o.close()
    if kind == "overlay":
        differs = 0
        for r, reset in c["oracle_reset"].items():
            keep = c["oracle"][r][0]
            for j in range(1, len(keep)):
                differs += int(keep[j][0][2] != reset[j][0][2])
                assert int(out["poses"][r][j].n_effect) == keep[j][0][2], (r, j)
        assert differs >= 1, "the oracle matches the same with and without the earlier scans' inserts"
    want = np.concatenate(worlds)
    got = out["cloud"][:, :3]
    pi = np.abs(body_in_imu(sc, np.concatenate(flat(c["runs"]))))
    tol = 1e-6 * (1.0 + pi.sum(axis=1, keepdims=True)) + ulp32(want)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{kind} {mode}: largest |cloud - oracle| {d.max():.3e} (largest share of its tolerance {np.max(d / tol):.3f})")
    assert np.all(d <= tol), (kind, mode, d.max(), np.max(d / tol))


def test_forms_write_the_same_bits(twin, clean_env):
    """5a. Run-resident against launch by launch (frozen: LEGKILO_RAGGED_LEVELS=1, which the message modes do not take; insert: LEGKILO_RAG_RESIDENT=0)."""
    c, out, kind, mode, g = twin["c"], twin["out"], twin["kind"], twin["mode"], twin["g"]
    if kind == "frozen":
        clean_env.setenv("LEGKILO_RAGGED_LEVELS", "1")
    else:
        assert twin["rounds"] >= 2, "no run stopped for the fallback launch: stop and resume are not exercised"
        clean_env.setenv("LEGKILO_RAG_RESIDENT", "0")
    got = cloud_call(g, kind, mode, c["runs"], c["tbs"], c["xs"], c["msgs"])
    if kind == "overlay":
        assert g.overlay_resident_rounds() == 0
    assert same_records(got["rec"], out["rec"]) and np.array_equal(got["sbo"], out["sbo"]), (kind, mode)
    assert same_cloud(got["cloud"], out["cloud"]), (kind, mode)
    assert tor.pose_bits(got["poses"]) == tor.pose_bits(out["poses"]) and np.array_equal(got["X"], out["X"]) and np.array_equal(got["P"], out["P"])


def large_overlay_runs(sc):
    """The CSR large-bucket case of test_overlay_runs.py: two runs of two dense scans of three buckets of 1 000 points."""
    rng = np.random.default_rng(6161)
    runs, tbs, xs = [], [], []
    for r in range(2):
        tb_run = [tor.T0 + 0.5 + 0.3 * r + tor.SCAN_GAP * j for j in range(2)]
        runs.append([synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=3000, n_buckets=3, seed_scan=8800 + 2 * r + j, seed_noise=8900 + 2 * r + j) for j, tb in enumerate(tb_run)])
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb_run[0], sc.P, rng, 0.02, 0.5))
    return runs, tbs, xs


@pytest.mark.parametrize("kind", KINDS)
def test_large_buckets(kind, store, oracle_lib, hip_lib, scene_plain):
    """5b. Buckets above 512 points take the launches: checks 2 and 3, and the existing entry's bits."""
    c = get_case(kind, "plain", store, oracle_lib, hip_lib, scene_plain)["c"]
    runs, tbs, xs = trr.large_runs(c["sc"]) if kind == "frozen" else large_overlay_runs(c["sc"])
    assert all(np.diff(synth.buckets_of(p)[0].astype(np.int64)).max() > 512 for run in runs for p in run)
    g = new_handle(hip_lib, c, 2)
    try:
        out = cloud_call(g, kind, "plain", runs, tbs, xs, None)
        if kind == "overlay":
            assert g.overlay_resident_rounds() == 0
            plain = g.batch_replay_overlay_runs(runs, tbs, xs, [P0] * 2)
        else:
            plain = g.batch_replay_runs(runs, tbs, xs, [P0] * 2)
        assert tor.pose_bits(plain) == tor.pose_bits(out["poses"])
        check_records(out, runs, tbs, ("large", kind))
        check_cloud(out, runs, c["sc"], f"large {kind}")
    finally:
        g.close()


def by_run(out, runs):
    """The table and the cloud run by run: [(records, cloud rows)]."""
    res, s, p = [], 0, 0
    for run in runs:
        n = sum(len(x) for x in run)
        res.append((out["rec"][int(out["sbo"][s]):int(out["sbo"][s + len(run)])], out["cloud"][p:p + n]))
        s, p = s + len(run), p + n
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_chunks(mode, k, store, oracle_lib, hip_lib, scene_plain):
    """6. Frozen map, the runs of two and more scans cut behind min(k, len - 1) scans (test_chunks_continue_bit_for_bit): records and clouds of the
    two calls, concatenated run by run, are the bits of the single call; a chunk's first_point counts in the chunk's own d_pts (check 2 on each chunk);
    the getters after the second call hold the second chunk only."""
    tw = get_case("frozen", mode, store, oracle_lib, hip_lib, scene_plain)
    c, g = tw["c"], tw["g"]
    idx = [r for r in range(len(c["runs"])) if len(c["runs"][r]) >= 2]
    runs, tbs, xs = [c["runs"][r] for r in idx], [c["tbs"][r] for r in idx], [c["xs"][r] for r in idx]
    msgs = None if c["msgs"] is None else [c["msgs"][r] for r in idx]
    if ("chunk_ref", mode) not in store:
        store[("chunk_ref", mode)] = cloud_call(g, "frozen", mode, runs, tbs, xs, msgs)
    ref = store[("chunk_ref", mode)]
    cut = [min(k, len(run) - 1) for run in runs]
    part = lambda nest, lo: None if nest is None else [n[:c_] if lo else n[c_:] for n, c_ in zip(nest, cut)]   # noqa: E731
    head = cloud_call(g, "frozen", mode, part(runs, True), part(tbs, True), xs, part(msgs, True))
    tail = cloud_call(g, "frozen", mode, part(runs, False), part(tbs, False), None, part(msgs, False), cont=True)
    check_records(head, part(runs, True), part(tbs, True), ("head", mode, k))
    check_records(tail, part(runs, False), part(tbs, False), ("tail", mode, k))
    joined = ([h + t for h, t in zip(head["poses"], tail["poses"])], tail["X"], tail["P"], tail["times"])
    assert trr.same_bits(joined, (ref["poses"], ref["X"], ref["P"], ref["times"])), (mode, k)
    for r, ((rr, rc), (hr, hc), (tr, tc)) in enumerate(zip(by_run(ref, runs), by_run(head, part(runs, True)), by_run(tail, part(runs, False)))):
        assert same_records(np.concatenate([hr, tr]), rr, first_point=False), (mode, k, r)
        assert same_cloud(np.concatenate([hc, tc]), rc), (mode, k, r)
    n_tail = int(tail["sbo"][-1])
    assert n_tail < int(ref["sbo"][-1]) and same_records(g.runs_bucket_poses(0, n_tail), tail["rec"])
    with pytest.raises(hip_lib.LegKiloError, match=INVALID):
        g.runs_bucket_poses(0, n_tail + 1)


@pytest.mark.parametrize("mode", MODES)
def test_pools_that_grow(mode, store, oracle_lib, hip_lib, scene_plain):
    """7. The overlay entry on a fresh handle's pools (test_pools_grow_and_refusals_leave_the_priors (a)): the four-scan run outgrows the first guess,
    the attempt loop runs the batch again.  Table and cloud are those of the calls behind it - the last of which leaves the pools as it found them, so
    it neither grew nor ran twice - and the shared case's."""
    tw = get_case("overlay", mode, store, oracle_lib, hip_lib, scene_plain)
    c = tw["c"]
    g = new_handle(hip_lib, c, len(c["runs"]))
    try:
        tor.device_call(g, c, runs=[c["runs"][2][:1]], tbs=[c["tbs"][2][:1]], xs=c["xs"][2:3], msgs=None if mode == "plain" else [c["msgs"][2][:1]])
        bytes1 = g.overlay_pool_bytes()
        first = cloud_call(g, "overlay", mode, c["runs"], c["tbs"], c["xs"], c["msgs"])
        bytes2 = g.overlay_pool_bytes()
        assert bytes2[1] > bytes1[1], "the four-scan run did not outgrow the first guess"
        second = cloud_call(g, "overlay", mode, c["runs"], c["tbs"], c["xs"], c["msgs"])   # (sized ahead of its attempt from the first call's high-water marks)
        bytes3 = g.overlay_pool_bytes()
        third = cloud_call(g, "overlay", mode, c["runs"], c["tbs"], c["xs"], c["msgs"])
        assert g.overlay_pool_bytes() == bytes3, "the pools still change: no call here ran on pools that were large enough from the start"
        for a in (second, third, tw["out"]):
            assert same_records(first["rec"], a["rec"]) and same_cloud(first["cloud"], a["cloud"]) and np.array_equal(first["sbo"], a["sbo"])
    finally:
        g.close()


def edge_runs(c):
    """Scans of 63, 64, 65, 1 and 257 points from the case's config-1 scans; the 65-point scan is ONE bucket of 65 points, the one-point scan one of 1."""
    src, stb = c["runs"][2], c["tbs"][2]   # config-1, one point, config-1 (clutter with the insert), config-1
    one65 = src[3][:65].copy()
    one65["curvature"] = one65["curvature"][0]
    big = c["runs"][0][0]
    assert len(big) >= 257 and len(src[1]) == 1
    runs = [[src[0][:63], src[0][63:127]], [one65, src[1]], [big[:257]]]
    assert [len(s) for run in runs for s in run] == [63, 64, 65, 1, 257]
    assert 65 in np.diff(synth.buckets_of(one65)[0].astype(np.int64))
    tbs = [[stb[0], stb[0] + tor.SCAN_GAP], [stb[3], stb[3] + tor.SCAN_GAP], [c["tbs"][0][0]]]
    return runs, tbs, [synth.initial_state(c["sc"].traj, tb_run[0], c["sc"].P) for tb_run in tbs]


@pytest.mark.parametrize("kind", KINDS)
def test_bounds(kind, store, oracle_lib, hip_lib, scene_plain):
    """8. d_world_out and lk_runs_bucket_poses_dev's d_out inside guard bands at offset 16: bands untouched, every record written; d_world_out NULL
    with scan_bucket_off; both NULL (nothing recorded)."""
    tw = get_case(kind, "plain", store, oracle_lib, hip_lib, scene_plain)
    c, g = tw["c"], tw["g"]
    runs, tbs, xs = edge_runs(c)
    ref = cloud_call(g, kind, "plain", runs, tbs, xs, None)
    check_records(ref, runs, tbs, ("edge", kind))
    check_cloud(ref, runs, c["sc"], f"edge {kind}")
    t = hip_lib.flatten_runs(runs, tbs)
    n, B = len(t["pts"]), int(ref["sbo"][-1])
    entry = g.batch_replay_runs_cloud_dev if kind == "frozen" else g.batch_replay_overlay_runs_cloud_dev
    args = (t["run_off"], t["scan_off"], t["t_begin"])
    gp = devguard.Guarded.input(g, t["pts"], offset=16, name="cloud d_pts")
    gw = devguard.Guarded(g, 16 * n, offset=16, name="d_world_out")
    gr = devguard.Guarded(g, REC.itemsize * B, offset=16, name="bucket poses d_out")
    arm = lambda: g.batch_set_priors(np.asarray(xs), np.asarray([P0] * len(runs)))   # noqa: E731
    try:
        arm()
        poses, sbo = entry(gp.ptr, *args, d_world=gw.ptr)
        cloud = gw.read(np.float32).reshape(n, 4)
        gp.check()
        assert devguard.sentinel_free(cloud) and same_cloud(cloud, ref["cloud"]) and np.array_equal(sbo, ref["sbo"])
        g.runs_bucket_poses_dev(0, B, gr.ptr)
        rec = gr.read(REC)
        assert devguard.sentinel_free(rec) and same_records(rec, ref["rec"]) and same_records(g.runs_bucket_poses(0, B), ref["rec"])
        gr.reset()
        g.runs_bucket_poses_dev(1, B - 2, gr.ptr)   # a range inside the table: its B - 2 records and nothing behind them
        got = gr.check()
        assert same_records(np.frombuffer(got[:REC.itemsize * (B - 2)].tobytes(), dtype=REC), ref["rec"][1:B - 1]) and devguard.untouched(got[REC.itemsize * (B - 2):])
        # the cloud not asked for: the table all the same, d_world_out's buffer left alone
        gw.reset()
        arm()
        poses2, sbo2 = entry(gp.ptr, *args, d_world=0)
        assert devguard.untouched(gw.check()) and np.array_equal(sbo2, ref["sbo"]) and same_records(g.runs_bucket_poses(0, B), ref["rec"])
        # neither output: the existing entry - same poses, and nothing recorded
        arm()
        poses3, none = entry(gp.ptr, *args, d_world=0, want_offsets=False)
        assert none is None and tor.pose_bits([poses3]) == tor.pose_bits([poses]) == tor.pose_bits([poses2]) == tor.pose_bits([flat(ref["poses"])])
        with pytest.raises(hip_lib.LegKiloError, match=STATE):
            g.runs_bucket_poses(0, 1)
        gp.check()
    finally:
        for b in (gp, gw, gr):
            b.free()


def test_refusals(store, oracle_lib, hip_lib, scene_plain):
    """9. LK_ERR_STATE from the getters on a fresh handle, after the plain run entry and after lk_batch_replay_dev; LK_ERR_INVALID for a range past the
    count and for a misaligned d_world_out (slots bit for bit as armed); a refusal of the wrapped entry keeps its message and the table."""
    tw = get_case("frozen", "plain", store, oracle_lib, hip_lib, scene_plain)
    c = tw["c"]
    runs, tbs, xs = c["runs"], c["tbs"], c["xs"]
    R = len(runs)
    g = new_handle(hip_lib, c, R)
    t = hip_lib.flatten_runs(runs, tbs)
    d_pts, d_world = g.device_malloc(t["pts"].nbytes), g.device_malloc(16 * len(t["pts"]) + 16)
    args = (t["run_off"], t["scan_off"], t["t_begin"])
    getters = (lambda a, n: g.runs_bucket_poses(a, n), lambda a, n: g.runs_bucket_poses_dev(a, n, d_world))

    def no_table(why):
        for get in getters:
            with pytest.raises(hip_lib.LegKiloError, match=STATE + ".*recorded no bucket poses"):
                get(0, 1)
        assert why

    try:
        g.h2d(d_pts, t["pts"])
        no_table("fresh handle")
        g.batch_set_priors(np.asarray(xs), np.asarray([P0] * R))
        _, sbo = g.batch_replay_runs_cloud_dev(d_pts, *args, d_world=d_world)
        B = int(sbo[-1])
        before = g.runs_bucket_poses(0, B)
        assert same_records(before, tw["out"]["rec"])
        for i, get in enumerate(getters):
            for a, n in ((0, B + 1), (B, 1), (B + 1, 0)) + (((1 << 63, 1 << 63),) if i else ()):   # (first + n wraps: no host array of that size to hand over)
                with pytest.raises(hip_lib.LegKiloError, match=INVALID + "bucket range"):
                    get(a, n)
        assert len(g.runs_bucket_poses(B, 0)) == 0
        # misaligned d_world_out: refused before the first write to a slot
        rng = np.random.default_rng(9191)
        Xa = np.array([synth.initial_state(c["sc"].traj, trr.T0 + r, c["sc"].P, rng, 0.02, 0.5) for r in range(R)])
        Pa = np.array([scenes.rand_spd(rng) for _ in range(R)]).reshape(R, 900)
        g.batch_set_priors(Xa, Pa)
        for r in range(R):
            g.set_times(10.0 + r, 9.5 + r, r)
        armed_t = trr.times_of(g, R)

        def as_armed(name):
            Xp, Pp = g.batch_get_states(0, R)
            assert np.array_equal(Xp, Xa) and np.array_equal(Pp.reshape(R, 900), Pa) and trr.times_of(g, R) == armed_t, name
            assert same_records(g.runs_bucket_poses(0, B), before), name

        for entry in (g.batch_replay_runs_cloud_dev, g.batch_replay_overlay_runs_cloud_dev):
            with pytest.raises(hip_lib.LegKiloError, match=INVALID + "d_world_out must be 16-byte aligned"):
                entry(d_pts, *args, d_world=d_world + 4)
            as_armed("misaligned")
        # a refusal of the wrapped entry: the same message, and the table still answers as it did
        empty_scan = t["scan_off"].copy()
        empty_scan[5] = empty_scan[4]
        for entry, plain in ((g.batch_replay_runs_cloud_dev, g.batch_replay_runs_dev), (g.batch_replay_overlay_runs_cloud_dev, g.batch_replay_overlay_runs_dev)):
            msgs = []
            for e, kw in ((plain, {}), (entry, dict(d_world=d_world))):
                with pytest.raises(hip_lib.LegKiloError, match=INVALID + "scan 4 is empty") as ei:
                    e(d_pts, t["run_off"], empty_scan, t["t_begin"], **kw)
                msgs.append(str(ei.value))
                as_armed("empty scan")
            assert msgs[0] == msgs[1]
        # the plain run entry and the uniform batch entry record nothing
        g.batch_set_priors(np.asarray(xs), np.asarray([P0] * R))
        g.batch_replay_runs_dev(d_pts, *args)
        no_table("after lk_batch_replay_runs_dev")
        g.batch_set_priors(np.asarray(xs), np.asarray([P0] * R))
        g.batch_replay_runs_cloud_dev(d_pts, *args, d_world=0)
        assert same_records(g.runs_bucket_poses(0, B), before)
        g.batch_set_priors(np.asarray(xs[:1]), np.asarray([P0]))
        off, dt = synth.buckets_of(runs[0][0])
        g.batch_replay_dev(d_pts, 1, len(runs[0][0]), tbs[0][0], off, dt)
        no_table("after lk_batch_replay_dev")
    finally:
        g.device_free(d_pts)
        g.device_free(d_world)
        g.close()
