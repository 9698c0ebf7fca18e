"""-m gpu: lk_batch_replay_overlay_runs_dev - whole recorded runs WITH the map insert, a run per filter slot, the slot's state, covariance, times
and overlay surviving the scan boundaries - against the CPU oracle's process_scan called scan after scan on a private copy of the map.

Setup (the idiom of test_batch_replay_overlay_ragged_scan_resident): a YOUNG map (first frame only, blob round-tripped), priors from
synth.initial_state(..., 0.02, 0.5), P = 1e-4 I, modes plain / imu / kin.  Six runs of 3, 1, 4, 2, 1, 3 scans: config-1 scans, one dense scan of
40 buckets, a one-point scan in the middle of a run, and config-1 scans with volumetric clutter - the insert's fallback items, what stops a run in
the resident launch - placed only as NON-first scans of their runs.  In the message modes every scan carries the stream over [tb, tb + 0.1] and,
at one boundary per run, the two record kinds of test_overlay_runs_pin.py: three records behind scan k's last bucket in scan k's package (never
applied) and one record of scan k + 1's package stamped 1 ms before scan k's last bucket time (applied at scan k + 1's first bucket).

Tolerances are those of the existing test for the same kernels on the same scene: counts exact, every scan's pose and the final state 1e-6,
covariance 1e-6 max|P|, compare_overlay rtol 1e-4 / ptol 2e-6 - but for the final STATE of a run of two or more scans, CHAIN_XTOL below.  The
device results and the oracle's are computed once per mode and shared by the cases.
"""
import numpy as np
import pytest

import scenes
from legkilo_amd import config, synth

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
MODES = ["plain", "imu", "kin"]
T0 = 2.0
RUN_SHAPES = [[None, "clutter", None], [(6000, 40)], [None, (1, 1), "clutter", None], [None, "clutter"], [None], [None, None, "clutter"]]
SCAN_GAP = 0.12   # a scan spans 0.1 s: 20 ms between a scan's last bucket and the next one's first
# Final state of a chain of scans against the oracle.  Measured on an MI355X: poses (rotation, position, velocity) 2.0e-7 at most in any scan of any
# run, the full 36-entry state 9.98e-7 in plain mode (run 5: three scans, the last with clutter; without messages biases and gravity are weakly
# observed and carry the chain's rounding differences), 3.2e-7 / 3.0e-7 / 2.8e-7 in the other plain chains, 1.6e-7 and 3.1e-8 at most with IMU and
# kinematic records; single-scan runs 1e-14.  The existing test's 1e-6 would hold by 0.2 %: the bound for chains is 5 x the measured value.
CHAIN_XTOL = 5e-6


def make_scan(sc, rng, shp, tb, k):
    if shp is None or shp == "clutter":
        pts = scenes.vlp_scan_input(sc, tb, 180 + k)
        if shp == "clutter":   # 30 cells of volumetric clutter in front of the robot, 60 points at a time in 30 of the scan's buckets (see the existing test)
            x = synth.initial_state(sc.traj, tb, sc.P)
            R0, p0 = x[:9].reshape(3, 3), x[9:12]
            eR, eT = np.asarray(sc.P["extrinsic_R"], dtype=np.float64).reshape(3, 3), np.asarray(sc.P["extrinsic_T"], dtype=np.float64)
            pw = scenes.corner_clutter(rng, n_cells=30, per_cell=60, origin=tuple(p0 + np.array([1.5, -1.0, -0.2])))
            pb = ((pw - p0) @ R0 - eT) @ eR
            cl = np.zeros(len(pb), dtype=synth.POINT_DTYPE)
            cl["x"], cl["y"], cl["z"] = pb[:, 0], pb[:, 1], pb[:, 2]
            stamps = np.unique(pts["curvature"])
            cl["curvature"] = stamps[((np.arange(len(pb)) // 60) * (len(stamps) // 31)) % len(stamps)]
            pts = np.concatenate([pts, cl])
            pts = pts[np.argsort(pts["curvature"], kind="stable")]
        return pts
    return synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=shp[0], n_buckets=shp[1], seed_scan=7600 + k, seed_noise=7700 + k)


def stream(sc, mode, tb, k):
    if mode == "imu":
        return synth.imu_stream(sc.traj, tb, tb + 0.1, seed=9500 + k)
    return synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=9600 + k)


def run_messages(sc, mode, runs, tbs, leftovers=True, lookback=True):
    """Messages per scan, nested like the runs (None in plain mode).  At the boundary behind the first scan of every run of >= 2 scans: (i) three
    records in scan 0's package behind its last bucket time and before scan 1's first bucket, (ii) one record in scan 1's package stamped 1 ms
    before scan 0's last bucket time."""
    if mode == "plain":
        return None
    stamp = "stamp" if mode == "imu" else "time_stamp"
    out, k = [], 0
    for run, tb_run in zip(runs, tbs):
        ms = []
        for j, (pts, tb) in enumerate(zip(run, tb_run)):
            m = stream(sc, mode, tb, k)
            if len(run) >= 2 and j < 2:
                last0 = tb_run[0] + float(run[0]["curvature"][-1])
                first1 = tb_run[1] + float(run[1]["curvature"][0])
                if j == 0:
                    m = m[m[stamp] < last0]   # (what the stream holds behind the last bucket goes with the leftovers)
                    if leftovers:
                        extra = m[-3:].copy()
                        extra[stamp] = last0 + (first1 - last0) * np.array([0.25, 0.5, 0.75])
                        assert np.all(extra[stamp] > last0) and np.all(extra[stamp] < first1)
                        m = np.concatenate([m, extra])
                elif lookback:
                    early = m[:1].copy()
                    early[stamp] = last0 - 1e-3
                    m = np.concatenate([early, m])
            assert np.all(np.diff(m[stamp]) > 0)
            ms.append(m)
            k += 1
        out.append(ms)
    return out


def young_map(oracle_lib, mode, scene_plain):
    if mode == "kin":
        sc = scenes.Scene(params=dict(config.DITER, voxel_grid_resolution=0.3), **CAPS)
    else:
        sc = scene_plain
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=(mode != "kin"))
    x0 = scenes.init_filter(o, sc, T0)
    scenes.first_frame(o, sc, T0, x0)   # a first frame only: most of what the scans see is new
    o.map_import(o.map_export())
    return sc, o, o.map_export()


def oracle_run(o, blob, x, P, run, tb_run, mode, msgs, reset_map=False):
    """KILO::process scan after scan on a private copy of the map; reset_map: the map is put back before every scan (state and times carried)."""
    o.map_import(blob)
    o.set_map_insert(True)
    o.set_state(x, P)
    o.set_times(tb_run[0], tb_run[0])
    poses = []
    for j, (pts, tb) in enumerate(zip(run, tb_run)):
        if reset_map and j > 0:
            xs_, Ps_ = o.get_state()
            tt = o.get_times()
            o.map_import(blob)
            o.set_map_insert(True)
            o.set_state(xs_, Ps_)
            o.set_times(*tt)
        kw = {} if mode == "plain" else {"imus" if mode == "imu" else "kins": msgs[j]}
        po, _ = o.process_scan(pts, tb, **kw)
        x_ = o.get_state()[0]
        poses.append(((po.n_buckets, po.n_updates, int(po.n_effect)), np.array(po.rot), np.array(po.pos), np.array(po.vel), x_.copy()))
    xo, Po = o.get_state()
    return poses, xo.copy(), Po.copy(), scenes.canon_map(o.map_export())


def msg_kw(mode, msgs):
    return {} if mode == "plain" else {"imus" if mode == "imu" else "kins": msgs}


def device_call(g, case, msgs=None, runs=None, tbs=None, xs=None):
    """One call of the entry from the case's priors -> (poses per run, states, covariances)."""
    runs = case["runs"] if runs is None else runs
    tbs = case["tbs"] if tbs is None else tbs
    xs = case["xs"] if xs is None else xs
    msgs = case["msgs"] if msgs is None else msgs
    poses = g.batch_replay_overlay_runs(runs, tbs, xs, [1e-4 * np.eye(30)] * len(runs), **msg_kw(case["mode"], msgs))
    X, P = g.batch_get_states(0, len(runs))
    return poses, X, P


def pose_bits(poses):
    return [(p.n_buckets, p.n_updates, int(p.n_effect), bytes(p.rot), bytes(p.pos), bytes(p.vel)) for run in poses for p in run]


@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**CAPS)


@pytest.fixture(scope="module")
def built():
    """The modes' cases as they are built (whatever order the tests come in, a mode is built once); their handles are closed behind the module."""
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


@pytest.fixture(params=MODES)
def case(request, built, oracle_lib, hip_lib, scene_plain):
    """Scans, messages, priors, the oracle's two passes and the device's result of one mode: computed once, shared by the cases, not changed."""
    if request.param not in built:
        built[request.param] = build_case(request.param, oracle_lib, hip_lib, scene_plain)
    return built[request.param]


def build_case(mode, oracle_lib, hip_lib, scene_plain):
    c = oracle_side(mode, oracle_lib, scene_plain)
    g = hip_lib.LegKiloHip(c["sc"].cfg(n_slots=len(c["runs"])))
    g.map_import(c["blob"])
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    c["g"] = g
    c["poses"], c["X"], c["P"] = device_call(g, c)
    c["rounds"] = g.overlay_resident_rounds()
    c["exports"] = [g.overlay_export(r) for r in range(len(c["runs"]))]
    return c


def oracle_side(mode, oracle_lib, scene_plain):
    sc, o, blob = young_map(oracle_lib, mode, scene_plain)
    o.set_acc_norm(9.81)
    rng = np.random.default_rng(828282)
    runs, tbs, xs, k = [], [], [], 0
    for r, shapes in enumerate(RUN_SHAPES):
        tb0 = T0 + 0.4 + 0.23 * r
        tb_run = [tb0 + SCAN_GAP * j for j in range(len(shapes))]
        run = []
        for shp, tb in zip(shapes, tb_run):
            run.append(make_scan(sc, rng, shp, tb, k))
            assert np.diff(synth.buckets_of(run[-1])[0].astype(np.int64)).max() <= 512
            k += 1
        runs.append(run)
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb0, sc.P, rng, 0.02, 0.5))
    msgs = run_messages(sc, mode, runs, tbs)
    c = dict(mode=mode, sc=sc, blob=blob, base=scenes.canon_map(blob), runs=runs, tbs=tbs, xs=xs, msgs=msgs)
    P0 = 1e-4 * np.eye(30)
    c["oracle"] = [oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], mode, None if msgs is None else msgs[r]) for r in range(len(runs))]
    c["oracle_reset"] = {r: oracle_run(o, blob, xs[r], P0, runs[r], tbs[r], mode, None if msgs is None else msgs[r], reset_map=True)[0]
                         for r in range(len(runs)) if len(runs[r]) >= 2}
    o.close()
    return c


@pytest.fixture()
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


def check_parity(case, poses, X, P, exports, tag):
    for r, (oposes, xo, Po, omap) in enumerate(case["oracle"]):
        for j, (cnt, rot, pos, vel, _) in enumerate(oposes):
            p = poses[r][j]
            assert (p.n_buckets, p.n_updates, int(p.n_effect)) == cnt, (tag, r, j, cnt, p.n_buckets, p.n_updates, p.n_effect)
            d = max(np.abs(np.array(p.rot) - rot).max(), np.abs(np.array(p.pos) - pos).max(), np.abs(np.array(p.vel) - vel).max())
            print(f"{tag} run {r} scan {j}: {len(case['runs'][r][j])} points, counts {cnt}, max |d pose| {d:.2e}")
            assert d < 1e-6, (tag, r, j, d)
        dx = np.abs(xo - X[r]).max()
        dP = np.abs(P[r] - Po).max() / np.abs(Po).max()
        print(f"{tag} run {r}: final max |dx| {dx:.2e}, |dP| / max|P| {dP:.2e}")
        assert dx < (CHAIN_XTOL if len(oposes) >= 2 else 1e-6), (tag, r, dx)
        assert dP <= 1e-6, (tag, r, dP)
        st = scenes.compare_overlay(exports[r], case["base"], omap, (tag, r), rtol=1e-4, ptol=2e-6)
        assert st["private_roots"] > 0


def test_runs_match_the_oracle_scan_after_scan(case, clean_env):
    """1. Per run: counts of every scan exact, every scan's pose and the final state to 1e-6, covariance to 1e-6 max|P|, every private voxel the
    oracle's.  The clutter really stops runs in the resident launch (>= 2 launches), in scans that are not their runs' first."""
    check_parity(case, case["poses"], case["X"], case["P"], case["exports"], case["mode"])
    assert case["rounds"] >= 2, f"no run stopped for the fallback launch ({case['rounds']} launch): the resume protocol is not exercised"


def test_the_overlay_persists_across_scan_boundaries(case, clean_env):
    """2. A second oracle pass puts the base map back before every scan (state and times carried).  It must match differently in some scan
    - shown by the oracle alone - and the device must equal the pass in which the map persists."""
    differs = 0
    for r, reset in case["oracle_reset"].items():
        keep = case["oracle"][r][0]
        assert reset[0][0] == keep[0][0], "the first scan of a run sees the base map either way"
        for j in range(1, len(keep)):
            differs += int(keep[j][0][2] != reset[j][0][2])
            p = case["poses"][r][j]
            assert int(p.n_effect) == keep[j][0][2], (r, j, int(p.n_effect), keep[j][0][2], reset[j][0][2])
    assert differs >= 1, "the oracle matches the same with and without the earlier scans' inserts: the scans do not show persistence"


@pytest.mark.parametrize("case", ["imu", "kin"], indirect=True)   # the message modes: the module's fixture of that mode
@pytest.mark.parametrize("which", ["leftovers", "lookback"])
def test_leftover_messages_are_dropped(case, clean_env, which):
    """3. Message modes: without the records behind a scan's last bucket the call gives the same bits; without the record of the next scan's
    package that is stamped before that bucket it does not."""
    g = case["g"]
    msgs = run_messages(case["sc"], case["mode"], case["runs"], case["tbs"], leftovers=which != "leftovers", lookback=which != "lookback")
    poses, X, P = device_call(g, case, msgs=msgs)
    same = np.array_equal(X, case["X"]) and np.array_equal(P, case["P"]) and pose_bits(poses) == pose_bits(case["poses"])
    if which == "leftovers":
        assert same, "records behind a scan's last bucket were applied in front of the next scan"
    else:
        assert not same, "a record of the next scan's package stamped before the last bucket of the scan before was skipped"
        multi = [r for r in range(len(case["runs"])) if len(case["runs"][r]) >= 2]
        assert all(not np.array_equal(X[r], case["X"][r]) for r in multi)
        single = [r for r in range(len(case["runs"])) if len(case["runs"][r]) == 1]
        assert all(np.array_equal(X[r], case["X"][r]) for r in single)


def test_resident_equals_launch_by_launch(case, clean_env):
    """4. LEGKILO_RAG_RESIDENT=0: bucket index after bucket index over the runs on the CSR tables - the bit-identity reference."""
    g = case["g"]
    clean_env.setenv("LEGKILO_RAG_RESIDENT", "0")
    poses, X, P = device_call(g, case)
    assert g.overlay_resident_rounds() == 0
    assert np.array_equal(X, case["X"]) and np.array_equal(P, case["P"]), "run-resident and launch-by-launch replay differ"
    assert pose_bits(poses) == pose_bits(case["poses"])
    for r in range(len(case["runs"])):
        assert scenes.maps_identical(g.overlay_export(r), case["exports"][r]), (case["mode"], r)


def test_runs_of_one_scan_are_the_existing_entry(case, clean_env):
    """5. n runs of one scan each through the new entry and the same scans through lk_batch_replay_overlay_ragged_dev: the same bits."""
    g, sc, mode = case["g"], case["sc"], case["mode"]
    pick = [(0, 0), (1, 0), (2, 1), (0, 1), (3, 0), (5, 2)]   # config-1, dense, one point, clutter, config-1, clutter
    scans = [case["runs"][r][j] for r, j in pick]
    tbs = [case["tbs"][r][j] for r, j in pick]
    msgs = None if mode == "plain" else [case["msgs"][r][j] for r, j in pick]
    rng = np.random.default_rng(5151)
    xs = [synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5) for tb in tbs]
    Ps = [1e-4 * np.eye(30)] * len(scans)
    poses_r = g.batch_replay_overlay_runs([[s] for s in scans], [[t] for t in tbs], xs, Ps, **msg_kw(mode, None if msgs is None else [[m] for m in msgs]))
    Xr, Pr = g.batch_get_states(0, len(scans))
    exp_r = [g.overlay_export(s) for s in range(len(scans))]
    poses_e = g.batch_replay_overlay_ragged(scans, tbs, xs, Ps, **msg_kw(mode, msgs))
    Xe, Pe = g.batch_get_states(0, len(scans))
    assert np.array_equal(Xr, Xe) and np.array_equal(Pr, Pe)
    assert pose_bits(poses_r) == pose_bits([[p] for p in poses_e])
    for s in range(len(scans)):
        assert scenes.maps_identical(g.overlay_export(s), exp_r[s]), (mode, s)


def test_large_buckets_take_the_launches_on_csr_tables(oracle_lib, hip_lib, scene_plain, clean_env):
    """6. Plain mode, two runs of two dense scans of three buckets of 1 000 points: above 512 points a bucket takes the launch-by-launch form
    (lk_rag_advance_kernel, residual, update, the insert passes, the pose tap) - on the device-built CSR tables.  Oracle parity as in case 1."""
    sc, o, blob = young_map(oracle_lib, "plain", scene_plain)
    rng = np.random.default_rng(6161)
    runs, tbs, xs = [], [], []
    for r in range(2):
        tb_run = [T0 + 0.5 + 0.3 * r + SCAN_GAP * j for j in range(2)]
        runs.append([synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=3000, n_buckets=3, seed_scan=8800 + 2 * r + j, seed_noise=8900 + 2 * r + j)
                     for j, tb in enumerate(tb_run)])
        assert all(np.diff(synth.buckets_of(p)[0].astype(np.int64)).max() > 512 for p in runs[-1])
        tbs.append(tb_run)
        xs.append(synth.initial_state(sc.traj, tb_run[0], sc.P, rng, 0.02, 0.5))
    c = dict(mode="plain", sc=sc, blob=blob, base=scenes.canon_map(blob), runs=runs, tbs=tbs, xs=xs, msgs=None)
    c["oracle"] = [oracle_run(o, blob, xs[r], 1e-4 * np.eye(30), runs[r], tbs[r], "plain", None) for r in range(2)]
    o.close()
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=2))
    g.map_import(blob)
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    poses, X, P = device_call(g, c)
    assert g.overlay_resident_rounds() == 0
    check_parity(c, poses, X, P, [g.overlay_export(r) for r in range(2)], "large")
    g.close()


def test_pools_grow_and_refusals_leave_the_priors(case, hip_lib, clean_env):
    """7. (a) a fresh handle with library-sized pools: the pools grow between a one-scan call and the call with the four-scan run, same bits as
    case 1; (b) pools set far too small, poisoned: a loud LK_ERR_CAPACITY, the slots at their priors; (c) library-sized again: case 1's bits;
    (d) argument errors: LK_ERR_INVALID naming the run / the scan, slots unchanged."""
    sc, mode, runs = case["sc"], case["mode"], case["runs"]
    R = len(runs)
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=R))
    g.map_import(case["blob"])
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    P0 = [1e-4 * np.eye(30)] * R
    # (a)
    one = device_call(g, case, runs=[runs[2][:1]], tbs=[case["tbs"][2][:1]], xs=case["xs"][2:3], msgs=None if mode == "plain" else [case["msgs"][2][:1]])
    assert len(one[0]) == 1
    bytes1 = g.overlay_pool_bytes()
    poses, X, P = device_call(g, case)
    bytes2 = g.overlay_pool_bytes()
    print(f"overlay pools {mode}: one scan {bytes1}, six runs {bytes2}; high-water marks {g.overlay_stats()}")
    assert bytes2[0] > bytes1[0]
    # (the oracle's map after the four-scan run holds ~6 000 changed voxels, a single scan's ~2 800; the first guess is 4 096 root entries either way)
    assert bytes2[1] > bytes1[1], "the four-scan run did not outgrow the first guess"
    assert np.array_equal(X, case["X"]) and np.array_equal(P, case["P"]) and pose_bits(poses) == pose_bits(case["poses"])
    # (b)
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    g.overlay_reserve(64, 128, 64)
    with pytest.raises(hip_lib.LegKiloError, match="overlay pool overflow"):
        device_call(g, case)
    clean_env.delenv("LEGKILO_POISON_POOLS", raising=False)
    Xp, Pp = g.batch_get_states(0, R)
    assert np.array_equal(Xp, np.array(case["xs"])) and np.array_equal(Pp, np.array(P0))
    # (c)
    g.overlay_reserve(0, 0, 0)
    poses, X, P = device_call(g, case)
    assert np.array_equal(X, case["X"]) and np.array_equal(P, case["P"]) and pose_bits(poses) == pose_bits(case["poses"])
    # (d)
    scans = [s for run in runs for s in run]
    run_off = np.r_[0, np.cumsum([len(run) for run in runs])].astype(np.uint32)
    scan_off = np.r_[0, np.cumsum([len(s) for s in scans])].astype(np.uint64)
    tb = [t for run in case["tbs"] for t in run]
    allpts = np.ascontiguousarray(np.concatenate(scans))
    bad = allpts.copy()
    i7 = int(scan_off[7]) + 5   # one decreasing curvature in scan 7
    bad["curvature"][i7] = bad["curvature"][i7 - 1] - np.float32(0.001)
    d_pts, d_bad = g.device_malloc(allpts.nbytes), g.device_malloc(bad.nbytes)
    g.h2d(d_pts, allpts)
    g.h2d(d_bad, bad)
    g.batch_set_priors(np.array(case["xs"]), np.array(P0))
    try:
        ro1 = run_off.copy()
        ro1[0] = 1
        empty = run_off.copy()
        empty[2] = empty[1]   # run 1 is empty
        for d, ro, pattern in ((d_pts, ro1, r"error -1: .*run_off\[0\]"), (d_pts, empty, r"error -1: run 1 is empty"),
                               (d_bad, run_off, r"error -1: scan 7 is not sorted"),
                               (d_pts, np.r_[run_off[:-1], run_off[-1] - 1, run_off[-1]].astype(np.uint32), r"error -1: n_runs")):
            with pytest.raises(hip_lib.LegKiloError, match=pattern):
                g.batch_replay_overlay_runs_dev(d, ro, scan_off, tb)
            Xp, Pp = g.batch_get_states(0, R)
            assert np.array_equal(Xp, np.array(case["xs"])) and np.array_equal(Pp, np.array(P0)), pattern
    finally:
        g.device_free(d_pts)
        g.device_free(d_bad)
    g.close()


def test_base_map_untouched_and_calls_repeat(case, clean_env):
    """8. The handle's map is what was imported, and a second identical call gives the same bits (the overlays start empty every time)."""
    g = case["g"]
    poses, X, P = device_call(g, case)
    assert np.array_equal(g.map_export(), np.frombuffer(case["blob"], dtype=np.uint8)) or scenes.maps_identical(g.map_export(), case["blob"])
    assert np.array_equal(X, case["X"]) and np.array_equal(P, case["P"]) and pose_bits(poses) == pose_bits(case["poses"])
    for r in range(len(case["runs"])):
        assert scenes.maps_identical(g.overlay_export(r), case["exports"][r]), (case["mode"], r)
