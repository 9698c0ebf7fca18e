"""-m gpu: lk_batch_replay_runs_dev - whole recorded runs on the FROZEN map, a run per filter slot, the slot's state, covariance and both time
stamps surviving the scan boundaries, LK_RUNS_CONTINUE to go on from what the slots hold - against the CPU oracle's process_scan called scan after
scan with set_map_insert(False) on the imported blob.

Setup: a map of first frame + 3 replayed scans (blob round-tripped), priors from synth.initial_state(..., 0.02, 0.5), P = 1e-4 I, modes plain / imu /
kin (kin on config.DITER).  Six runs of 3, 1, 4, 2, 1, 3 scans: config-1 scans, dense scans of 40 buckets and a one-point scan in the middle of a
run.  In the message modes every scan carries the stream over [tb, tb + 0.1] and, at the first boundary of every run, the two record kinds of
test_overlay_runs_pin.py (run_messages of test_overlay_runs.py): three records behind scan 0's last bucket in scan 0's package (never applied) and
one record of scan 1's package stamped 1 ms before scan 0's last bucket time (applied at scan 1's first bucket).

Tolerances are test_overlay_runs.py's, the project's measured bounds for the same filter cores: counts exact, every scan's pose 1e-6, the final state
1e-6 for one-scan runs and CHAIN_XTOL for chains, covariance 1e-6 max|P|.  The oracle's passes and the device's result are computed once per mode and
shared by the cases.  Sensitivity, shown by the oracle alone before any device run: with the oracle's insert ON the same runs match differently in
some non-first scan - a device path that inserted could not pass the count checks.
"""
import numpy as np
import pytest

import devguard
import scenes
import test_overlay_runs as tor   # make_scan, run_messages, msg_kw, pose_bits, the tolerances
from legkilo_amd import config, synth

pytestmark = pytest.mark.gpu

CAPS = tor.CAPS
MODES = tor.MODES
T0 = 2.0
MAP_SCANS = 3
RUN_SHAPES = [[None, None, None], [(6000, 40)], [None, (1, 1), None, None], [None, None], [None], [None, (6000, 40), None]]
SCAN_GAP = tor.SCAN_GAP
CHAIN_XTOL = tor.CHAIN_XTOL
P0 = 1e-4 * np.eye(30)
BIG_MSG = "only replayed for scans whose buckets hold <= 512 points"


def mature_map(oracle_lib, mode, scene_plain):
    """First frame + MAP_SCANS scans replayed live on the oracle: mature enough that the runs' scans match."""
    sc = scenes.Scene(params=dict(config.DITER, voxel_grid_resolution=0.3), **CAPS) if mode == "kin" else scene_plain
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=(mode != "kin"))
    x0 = scenes.init_filter(o, sc, T0)
    scenes.first_frame(o, sc, T0, x0)
    scenes.replay_vlp(o, sc, T0, MAP_SCANS, use_kin=(mode == "kin"))
    o.map_import(o.map_export())
    return sc, o, o.map_export()


def oracle_run(o, blob, x, P, run, tb_run, mode, msgs, insert=False):
    """KILO::process scan after scan on the imported blob, state and times carried; insert: the map grows (the sensitivity pass)."""
    o.map_import(blob)
    o.set_map_insert(insert)
    o.set_state(x, P)
    o.set_times(tb_run[0], tb_run[0])
    poses = []
    for j, (pts, tb) in enumerate(zip(run, tb_run)):
        kw = {} if mode == "plain" else {"imus" if mode == "imu" else "kins": msgs[j]}
        po, _ = o.process_scan(pts, tb, **kw)
        poses.append(((po.n_buckets, po.n_updates, int(po.n_effect)), np.array(po.rot), np.array(po.pos), np.array(po.vel)))
    xo, Po = o.get_state()
    return poses, xo.copy(), Po.copy()


def new_handle(hip_lib, sc, blob, n_slots, **over):
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=n_slots, **over))
    g.map_import(blob)
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    return g


def times_of(g, n):
    return [g.get_times(r) for r in range(n)]


def device_call(g, mode, runs, tbs, xs, msgs, cont=False):
    """One call of the entry (from the priors xs, or continued) -> (poses per run, states, covariances, times)."""
    poses = g.batch_replay_runs(runs, tbs, None if cont else xs, None if cont else [P0] * len(runs), cont=cont, **tor.msg_kw(mode, msgs))
    X, P = g.batch_get_states(0, len(runs))
    return poses, X, P, times_of(g, len(runs))


def same_bits(a, b):
    return tor.pose_bits(a[0]) == tor.pose_bits(b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


@pytest.fixture(params=MODES)
def case(request, built, oracle_lib, hip_lib, scene_plain):
    """Scans, messages, priors, the oracle's two passes and the device's result of one mode: computed once, shared by the cases, not changed."""
    return build_case(request.param, built, oracle_lib, hip_lib, scene_plain)


def build_case(mode, built, oracle_lib, hip_lib, scene_plain):
    if mode not in built:
        c = oracle_side(mode, oracle_lib, scene_plain)
        c["g"] = new_handle(hip_lib, c["sc"], c["blob"], len(c["runs"]))
        c["map_before"] = c["g"].map_export().copy()
        c["dev"] = device_call(c["g"], c["mode"], c["runs"], c["tbs"], c["xs"], c["msgs"])
        built[mode] = c
    return built[mode]


def oracle_side(mode, oracle_lib, scene_plain):
    sc, o, blob = mature_map(oracle_lib, mode, scene_plain)
    o.set_acc_norm(9.81)
    rng = np.random.default_rng(919191)
    runs, tbs, xs, k = [], [], [], 0
    for r, shapes in enumerate(RUN_SHAPES):
        tb0 = T0 + 0.1 * (MAP_SCANS + 1) + 0.23 * r
        tb_run = [tb0 + SCAN_GAP * j for j in range(len(shapes))]
        run = []
        for shp, tb in zip(shapes, tb_run):
            run.append(tor.make_scan(sc, rng, shp, tb, k))
            assert np.diff(synth.buckets_of(run[-1])[0].astype(np.int64)).max() <= 512
            k += 1
        runs.append(run)
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb0, sc.P, rng, 0.02, 0.5))
    msgs = tor.run_messages(sc, mode, runs, tbs)
    c = dict(mode=mode, sc=sc, blob=blob, runs=runs, tbs=tbs, xs=xs, msgs=msgs)
    mr = lambda r: None if msgs is None else msgs[r]   # noqa: E731
    c["oracle"] = [oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], mode, mr(r)) for r in range(len(runs))]
    # sensitivity, on the CPU with the oracle alone: with the insert ON some non-first scan of some run matches differently
    differs = 0
    for r in range(len(runs)):
        if len(runs[r]) >= 2:
            grown = oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], mode, mr(r), insert=True)[0]
            differs += sum(int(grown[j][0][2] != c["oracle"][r][0][j][0][2]) for j in range(1, len(runs[r])))
    assert differs >= 1, "the oracle matches the same with and without the insert: these runs cannot tell a frozen map from a growing one"
    assert all(op[0][j][0][2] > 0 for r, op in enumerate(c["oracle"]) for j in range(len(runs[r])) if len(runs[r][j]) > 1), "a scan matches nothing: the map is too young"
    o.close()
    return c


@pytest.fixture()
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_RAGGED_LEVELS", raising=False)
    return monkeypatch


def check_parity(oracle, runs, poses, X, P, tag):
    for r, (oposes, xo, Po) in enumerate(oracle):
        for j, (cnt, rot, pos, vel) in enumerate(oposes):
            p = poses[r][j]
            d = max(np.abs(np.array(p.rot) - rot).max(), np.abs(np.array(p.pos) - pos).max(), np.abs(np.array(p.vel) - vel).max())
            print(f"{tag} run {r} scan {j}: {len(runs[r][j])} points, counts {cnt} / device {(p.n_buckets, p.n_updates, int(p.n_effect))}, max |d pose| {d:.2e}")
            assert (p.n_buckets, p.n_updates, int(p.n_effect)) == cnt, (tag, r, j, cnt, p.n_buckets, p.n_updates, p.n_effect)
            assert d < 1e-6, (tag, r, j, d)
        dx = np.abs(xo - X[r]).max()
        dP = np.abs(P[r] - Po).max() / np.abs(Po).max()
        print(f"{tag} run {r}: final max |dx| {dx:.2e}, |dP| / max|P| {dP:.2e}")
        assert dx < (CHAIN_XTOL if len(oposes) >= 2 else 1e-6), (tag, r, dx)
        assert dP <= 1e-6, (tag, r, dP)


def test_runs_match_the_oracle_on_the_frozen_map(case, clean_env):
    """1. Per run: counts of every scan exact, every scan's pose 1e-6, the final state 1e-6 (one scan) / CHAIN_XTOL (chains), covariance 1e-6 max|P|;
    the slots' counters are the last scans'."""
    poses, X, P, _ = case["dev"]
    check_parity(case["oracle"], case["runs"], poses, X, P, case["mode"])


def test_the_map_stays_frozen(case, clean_env):
    """2. map_export is byte-equal before and after (and after one more call, which gives the same bits)."""
    g = case["g"]
    again = device_call(g, case["mode"], case["runs"], case["tbs"], case["xs"], case["msgs"])
    assert same_bits(again, case["dev"])
    assert np.array_equal(g.map_export(), case["map_before"])


@pytest.mark.parametrize("case", ["imu", "kin"], indirect=True)
@pytest.mark.parametrize("which", ["leftovers", "lookback"])
def test_boundary_rules(case, clean_env, which):
    """3. Without the records behind a scan's last bucket the call gives the same bits; without the record of the next scan's package that is
    stamped before that bucket, the pose of the scan behind the boundary changes."""
    msgs = tor.run_messages(case["sc"], case["mode"], case["runs"], case["tbs"], leftovers=which != "leftovers", lookback=which != "lookback")
    got = device_call(case["g"], case["mode"], case["runs"], case["tbs"], case["xs"], msgs)
    if which == "leftovers":
        assert same_bits(got, case["dev"]), "records behind a scan's last bucket were applied in front of the next scan"
        return
    for r, run in enumerate(case["runs"]):
        a, b = tor.pose_bits([got[0][r]]), tor.pose_bits([case["dev"][0][r]])
        assert a[0] == b[0], "the first scan's package is the same"
        if len(run) >= 2:
            assert a[1][3:] != b[1][3:], (r, "a record of the next scan's package stamped before the last bucket of the scan before was skipped")
        else:
            assert np.array_equal(got[1][r], case["dev"][1][r])


@pytest.fixture(scope="module")
def chunk_refs():
    return {}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_chunks_continue_bit_for_bit(case, clean_env, chunk_refs, k):
    """4. The runs of two and more scans (one of four among them), run r cut behind min(k, len - 1) scans: the first part with flags 0 and the
    rest with LK_RUNS_CONTINUE give the bits of one call - every scan's pose, states, covariances, both time stamps.  In imu mode: the second
    call WITHOUT the flag does not."""
    g, mode = case["g"], case["mode"]
    idx = [r for r in range(len(case["runs"])) if len(case["runs"][r]) >= 2]
    assert max(len(case["runs"][r]) for r in idx) == 4
    runs, tbs, xs = [case["runs"][r] for r in idx], [case["tbs"][r] for r in idx], [case["xs"][r] for r in idx]
    msgs = None if case["msgs"] is None else [case["msgs"][r] for r in idx]
    if mode not in chunk_refs:
        chunk_refs[mode] = device_call(g, mode, runs, tbs, xs, msgs)
    ref = chunk_refs[mode]
    cut = [min(k, len(run) - 1) for run in runs]
    part = lambda nest, lo: None if nest is None else [n[:c] if lo else n[c:] for n, c in zip(nest, cut)]   # noqa: E731
    head = device_call(g, mode, part(runs, True), part(tbs, True), xs, part(msgs, True))
    tail = device_call(g, mode, part(runs, False), part(tbs, False), None, part(msgs, False), cont=True)
    joined = ([h + t for h, t in zip(head[0], tail[0])],) + tail[1:]
    assert same_bits(joined, ref), (mode, k)
    if mode == "imu":
        device_call(g, mode, part(runs, True), part(tbs, True), xs, part(msgs, True))
        g.batch_replay_runs(part(runs, False), part(tbs, False), imus=part(msgs, False))   # flags 0, no priors: state kept, times reset
        X, _ = g.batch_get_states(0, len(runs))   # (the time stamps END where they do either way: at the runs' last bucket times)
        assert all(not np.array_equal(X[r], ref[1][r]) for r in range(len(runs))), "the second call went on from the held time stamps without the flag"


def test_runs_of_one_scan_are_the_scan_entries(case, clean_env):
    """5. n runs of one scan each and the same scans through lk_batch_replay_scans_dev (and _imu_dev / _kin_dev from device records): the same bits."""
    g, sc, mode = case["g"], case["sc"], case["mode"]
    pick = [(0, 0), (1, 0), (2, 1), (0, 1), (3, 0), (5, 1)]   # config-1, dense, one point, config-1, config-1, dense
    scans = [case["runs"][r][j] for r, j in pick]
    tbs = [case["tbs"][r][j] for r, j in pick]
    msgs = None if mode == "plain" else [case["msgs"][r][j] for r, j in pick]
    rng = np.random.default_rng(5151)
    xs = [synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5) for tb in tbs]
    n = len(scans)
    one = device_call(g, mode, [[s] for s in scans], [[t] for t in tbs], xs, None if msgs is None else [[m] for m in msgs])
    poses_e = g.batch_replay_ragged(scans, tbs, xs, [P0] * n, **tor.msg_kw(mode, msgs))
    Xe, Pe = g.batch_get_states(0, n)
    assert same_bits(one, ([[p] for p in poses_e], Xe, Pe, times_of(g, n)))
    if mode != "plain":
        allpts, allmsg = np.ascontiguousarray(np.concatenate(scans)), np.ascontiguousarray(np.concatenate(msgs))
        d_pts, d_msg = g.device_malloc(allpts.nbytes), g.device_malloc(allmsg.nbytes)
        try:
            g.h2d(d_pts, allpts)
            g.h2d(d_msg, allmsg)
            g.batch_set_priors(np.asarray(xs), np.asarray([P0] * n))
            entry = g.batch_replay_scans_imu_dev if mode == "imu" else g.batch_replay_scans_kin_dev
            poses_d = entry(d_pts, np.r_[0, np.cumsum([len(s) for s in scans])], tbs, np.array([len(m) for m in msgs], dtype=np.uint32), d_msg)
            Xd, Pd = g.batch_get_states(0, n)
            assert same_bits(one, ([[p] for p in poses_d], Xd, Pd, times_of(g, n)))
        finally:
            g.device_free(d_pts)
            g.device_free(d_msg)


def test_resident_equals_launch_by_launch(built, oracle_lib, hip_lib, scene_plain, clean_env):
    """6a. Plain mode: LEGKILO_RAGGED_LEVELS=1 (residual, update, pose tap + predict per bucket index) gives the run-resident kernel's bits."""
    c = build_case("plain", built, oracle_lib, hip_lib, scene_plain)
    clean_env.setenv("LEGKILO_RAGGED_LEVELS", "1")
    got = device_call(c["g"], "plain", c["runs"], c["tbs"], c["xs"], None)
    assert same_bits(got, c["dev"]), "run-resident and launch-by-launch replay differ"


def large_runs(sc, n_runs=2):
    rng = np.random.default_rng(6161)
    runs, tbs, xs = [], [], []
    for r in range(n_runs):
        tb_run = [T0 + 0.1 * (MAP_SCANS + 1) + 0.3 * r + SCAN_GAP * j for j in range(2)]
        runs.append([synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=4000, n_buckets=4, seed_scan=8800 + 2 * r + j, seed_noise=8900 + 2 * r + j)
                     for j, tb in enumerate(tb_run)])
        assert all(np.diff(synth.buckets_of(p)[0].astype(np.int64)).max() > 512 for p in runs[-1])
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb_run[0], sc.P, rng, 0.02, 0.5))
    return runs, tbs, xs


def test_large_buckets_take_the_launches(oracle_lib, hip_lib, scene_plain, clean_env):
    """6b. Plain mode, two runs of two dense scans of four buckets of 1 000 points: above 512 points a bucket takes the launch-by-launch form.
    Oracle parity at the bounds of case 1."""
    sc, o, blob = mature_map(oracle_lib, "plain", scene_plain)
    runs, tbs, xs = large_runs(sc)
    oracle = [oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], "plain", None) for r in range(2)]
    o.close()
    g = new_handle(hip_lib, sc, blob, 2)
    poses, X, P, _ = device_call(g, "plain", runs, tbs, xs, None)
    g.close()
    check_parity(oracle, runs, poses, X, P, "large")


def test_refusals_leave_the_slots_as_they_were(case, hip_lib, clean_env):
    """7. Every LK_ERR_INVALID (-1) / LK_ERR_CAPACITY case of the header; the unsorted-scan and empty-scan messages name the scan; messages with
    a bucket above 512 points are refused; after each refusal states, covariances and times are what was armed, bit for bit."""
    sc, mode, runs = case["sc"], case["mode"], case["runs"]
    R = len(runs)
    g = new_handle(hip_lib, sc, case["blob"], R)
    t = hip_lib.flatten_runs(runs, case["tbs"])
    run_off, scan_off, tb, allpts = t["run_off"], t["scan_off"], t["t_begin"], t["pts"]
    S = len(tb)
    bad = allpts.copy()
    i7 = int(scan_off[7]) + 5   # one decreasing curvature in scan 7
    bad["curvature"][i7] = bad["curvature"][i7 - 1] - np.float32(0.001)
    big_runs, big_tbs, _ = large_runs(sc, 1)
    tbig = hip_lib.flatten_runs(big_runs, big_tbs, imus=[[synth.imu_stream(sc.traj, b, b + 0.1, seed=77 + j) for j, b in enumerate(big_tbs[0])]])
    d_pts, d_bad, d_big, d_bigm = (g.device_malloc(a.nbytes) for a in (allpts, bad, tbig["pts"], tbig["msgs"]))
    for d, a in ((d_pts, allpts), (d_bad, bad), (d_big, tbig["pts"]), (d_bigm, tbig["msgs"])):
        g.h2d(d, a)
    rng = np.random.default_rng(7171)
    Xa = np.array([synth.initial_state(sc.traj, T0 + r, sc.P, rng, 0.02, 0.5) for r in range(R)])
    Pa = np.array([scenes.rand_spd(rng) for _ in range(R)]).reshape(R, 900)
    g.batch_set_priors(Xa, Pa)
    for r in range(R):
        g.set_times(10.0 + r, 9.5 + r, r)
    armed_t = times_of(g, R)
    ro1 = run_off.copy()
    ro1[0] = 1
    empty_run = run_off.copy()
    empty_run[2] = empty_run[1]
    empty_scan = scan_off.copy()
    empty_scan[5] = empty_scan[4]
    half = np.full(2, 1 << 31, dtype=np.uint32)
    two = dict(run_off=[0, 2], scan_off=scan_off[:3], t_begins=tb[:2])
    cases = [
        ("n_runs 0", dict(run_off=[0]), r"error -1: n_runs"),
        ("n_runs above n_slots", dict(run_off=np.r_[run_off[:-1], run_off[-1] - 1, run_off[-1]]), r"error -1: n_runs"),
        ("run_off[0]", dict(run_off=ro1), r"error -1: .*run_off\[0\]"),
        ("empty run", dict(run_off=empty_run), r"error -1: run 1 is empty"),
        ("empty scan", dict(scan_off=empty_scan), r"error -1: scan 4 is empty"),
        ("unsorted scan", dict(d_pts=d_bad), r"error -1: scan 7 is not sorted"),
        ("msg_kind 3", dict(msg_kind=3, n_msg=np.zeros(S, dtype=np.uint32)), r"error -1: msg_kind"),
        ("msg_kind without n_msg", dict(msg_kind=1), r"error -1: msg_kind"),
        ("null points", dict(d_pts=0), r"error -1: null argument"),
        ("null messages", dict(msg_kind=1, n_msg=np.ones(S, dtype=np.uint32)), r"error -1: null message array"),
        ("unknown flag bits", dict(flags=2), r"error -1: unknown flag"),
        ("unknown flag bits with the known one", dict(flags=5), r"error -1: unknown flag"),
        ("messages with a bucket above 512 points", dict(d_pts=d_big, run_off=tbig["run_off"], scan_off=tbig["scan_off"], t_begins=tbig["t_begin"], msg_kind=1,
                                                         n_msg=tbig["n_msg"], d_msgs=d_bigm), "error -1: .*" + BIG_MSG),
        ("2^32 points", dict(run_off=[0, 1], scan_off=np.array([0, 1 << 32], dtype=np.uint64), t_begins=tb[:1]), r"error -3: more than 2\^32 points"),
        ("2^32 messages", dict(msg_kind=1, n_msg=half, d_msgs=d_pts, **two), r"error -3: more than 2\^32 messages"),
    ]
    try:
        for name, over, pattern in cases:
            kw = dict(d_pts=d_pts, run_off=run_off, scan_off=scan_off, t_begins=tb)
            kw.update(over)
            with pytest.raises(hip_lib.LegKiloError, match=pattern):
                g.batch_replay_runs_dev(**kw)
            Xp, Pp = g.batch_get_states(0, R)
            assert np.array_equal(Xp, Xa) and np.array_equal(Pp.reshape(R, 900), Pa) and times_of(g, R) == armed_t, name
    finally:
        for d in (d_pts, d_bad, d_big, d_bigm):
            g.device_free(d)
        g.close()
    # a bucket above max_scan_points: a handle of its own (512 points per scan at most, buckets of 1 000)
    g = new_handle(hip_lib, sc, case["blob"], 1, max_scan_points=512)
    g.batch_set_priors(Xa[:1], Pa[:1])
    g.set_times(10.0, 9.5, 0)
    with pytest.raises(hip_lib.LegKiloError, match=r"error -3: bucket exceeds max_scan_points"):
        g.batch_replay_runs(big_runs, big_tbs)
    Xp, Pp = g.batch_get_states(0, 1)
    assert np.array_equal(Xp, Xa[:1]) and np.array_equal(Pp.reshape(1, 900), Pa[:1]) and g.get_times(0) == (10.0, 9.5)
    g.close()


@pytest.mark.parametrize("case", ["imu", "kin"], indirect=True)
def test_guard_bands(case, hip_lib, clean_env):
    """8. Guard bands around d_pts and d_msgs, scans of 63 / 64 / 65 points and a run whose last scan has one point: bands intact, inputs
    unchanged, results those of the unguarded call."""
    g, mode = case["g"], case["mode"]
    src, stb, smsg = case["runs"][2], case["tbs"][2], case["msgs"][2]   # config-1, one point, config-1, config-1
    runs = [[src[0][:63], src[2][:64]], [src[3][:65], src[1]]]
    assert [len(s) for run in runs for s in run] == [63, 64, 65, 1]
    tbs = [[stb[0], stb[2]], [stb[3], stb[3] + SCAN_GAP]]
    msgs = [[smsg[0], smsg[2]], [smsg[3], smsg[1][:0]]]   # (the one-point scan: an empty package at the end of the message array)
    xs = [case["xs"][2], case["xs"][3]]
    ref = device_call(g, mode, runs, tbs, xs, msgs)
    t = hip_lib.flatten_runs(runs, tbs, **tor.msg_kw(mode, msgs))
    gp = devguard.Guarded.input(g, t["pts"], offset=16, name="runs d_pts")
    gm = devguard.Guarded.input(g, t["msgs"], offset=8, name="runs d_msgs")
    try:
        g.batch_set_priors(np.asarray(xs), np.asarray([P0] * 2))
        flat = g.batch_replay_runs_dev(gp.ptr, t["run_off"], t["scan_off"], t["t_begin"], t["msg_kind"], t["n_msg"], gm.ptr)
        gp.check()
        gm.check()
        X, P = g.batch_get_states(0, 2)
        assert same_bits(([flat[:2], flat[2:]], X, P, times_of(g, 2)), ref)
    finally:
        gp.free()
        gm.free()

